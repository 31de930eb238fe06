"""Child-process body of the two-rank finite-shot GPU test (not a test module); started from the forkserver of
conftest.py like shard_worker.py's ranks."""
import os
import traceback

import numpy as np

from shard_worker import _init


def shots_rank(rank, world_size, port, n, L, out_dir):
    """One rank of a shots-mode KSD-gradient step under a real gloo group: interleaved deal of the shifted circuits,
    each sampled with its global circuit id, all-gather of the gradient scalars."""
    try:
        _init(rank, world_size, port)
        import torch
        import torch.distributed as dist
        dist.init_process_group("gloo", rank=rank, world_size=world_size)
        try:
            from tensornetworks_amd.bayesian_network import synthetic_network
            from tensornetworks_amd.ksd_vi_quantum import KSDVariationalInference
            torch.cuda.set_device(0)
            bn, lat, obs, x = synthetic_network(n, seed=1)
            torch.manual_seed(7)
            vi = KSDVariationalInference(bn, lat, obs, qbm_num_latent_vars=n, qbm_ansatz_layers=L, pytorch_device="cuda:0",
                                         gram_mode="kron", qbm_shots=3000, shot_seed=123)
            vi._prepare_stein(x)
            loss, grad, q = vi.ksd_and_grad()
            torch.cuda.synchronize()
            np.savez(os.path.join(out_dir, f"rank{rank}.npz"), loss=loss.cpu().numpy(), grad=grad.cpu().numpy(),
                     q=q.cpu().numpy())
            dist.barrier()
        finally:
            dist.destroy_process_group()
    except BaseException:
        with open(os.path.join(out_dir, f"rank{rank}.err"), "w") as f:
            traceback.print_exc(file=f)
        raise
