"""Child-process body of tests/test_gpu_plan_commute.py (not a test module); started from the forkserver of conftest.py
like shard_worker.py's ranks, so that the batch below is the FIRST GPU work of its process."""
import hashlib
import os
import traceback

import numpy as np


def cold_rows(rank, world_size, port, n, L, reg_wires, out_dir):
    """hardware_efficient, default tiles: the full parameter-shift batch as stored rows (prefix sharing off, then on), and
    -- where the plan has it -- the fused dot against the gradient of the stored rows.  The parent checks what comes back."""
    try:
        import torch
        from tensornetworks_amd import backend as be
        ansatz = "hardware_efficient"
        dev = torch.device("cuda", 0)
        be.set_option(dev, "reg_wires", int(reg_wires))
        be.set_option(dev, "prefix_share", 0)
        P = be.num_params(ansatz, n, L)
        rng = np.random.default_rng([n, L, 5])
        theta = rng.uniform(-np.pi, np.pi, P)
        th = torch.from_numpy(theta).to(dev)
        full = be.paramshift_probs(ansatz, n, L, th, 0, P, include_base=True).clone()      # the first launches of the process
        picks = [0, P // 2 + 1, P - 1]
        rows = [0] + [r for p_ in picks for r in (1 + 2 * p_, 2 + 2 * p_)]
        out = {"theta": theta, "picks": np.array(picks), "rows": full[rows].cpu().numpy(),
               "worst_sum": np.float64(float((full.sum(dim=1) - 1.0).abs().max())),
               "digest": np.array(hashlib.sha256(full.cpu().numpy().tobytes()).hexdigest())}
        be.set_option(dev, "prefix_share", 1)
        shared = be.paramshift_probs(ansatz, n, L, th, 0, P, include_base=True)
        out["digest_shared"] = np.array(hashlib.sha256(shared.cpu().numpy().tobytes()).hexdigest())
        be.set_option(dev, "prefix_share", 0)
        fused = bool(be.paramshift_dot_supported(ansatz, n, L, dev, P))
        out["fused"] = np.array(fused)
        if fused:
            w = torch.from_numpy(rng.standard_normal(1 << n)).to(dev)
            ksd2 = torch.tensor([3.7], dtype=torch.float64, device=dev)
            loss_u, grad_u, _ = be.ksd_grad_finish(n, full[1:], P, w, ksd2)
            q, tok = be.paramshift_dot_begin(ansatz, n, L, th, 0, P)
            loss_f, grad_f = be.paramshift_dot_finish(tok, w, ksd2)
            out.update(q_equal=np.array(bool(torch.equal(q, full[0]))), loss_equal=np.array(bool(torch.equal(loss_f, loss_u))),
                       grad_fused=grad_f.cpu().numpy(), grad_stored=grad_u.cpu().numpy())
        np.savez(os.path.join(out_dir, f"cold_{n}_{L}_{reg_wires}.npz"), **out)
    except BaseException:
        with open(os.path.join(out_dir, f"rank{rank}.err"), "w") as f:
            traceback.print_exc(file=f)
        raise
