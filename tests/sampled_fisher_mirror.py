"""Oracle of the sampled natural gradient of the MPS Born machine (test infrastructure, plain NumPy / CPU torch, not under
test).  Conventions of mps_sampled_mirror; np.longdouble where hp_reference.HAVE_LONGDOUBLE holds, no rescaling.

  score_rows     o_b[k, s, a, c] = 2 [z_bk = s] l_b,k-1[a] r_b,k[c] / psi_b - mu[k, s, a, c],  mu = 2 (L_k-1 A_k[s] E_k)[a][c] / Z,
                 as rows [n, 2 D^2, B], and `rows_abs`: every term's magnitude (|cores|, + for -, divided by the true |psi_b|
                 and the true Z), the value the kernels' error bounds are expressed in
  fisher         F^ = (1 / B) sum_b o_b o_b^T: the n site blocks [n, R, R] and the whole matrix [P, P], each with the sum of
                 the products' magnitudes
  exact_fisher   sum_z q_z o_z o_z^T over all 2^n outcomes (small n)
  damped_solve   (F + damping I)^-1 g by Cholesky in the mirror's arithmetic; None where a pivot is not positive
  precondition   delta [n, 2, D, D] and the per-block infos (0, or 1 where the factorisation failed: that block of delta is g)
  replay         float64 restatement of the sampled trainers' epochs with the preconditioner, from mps_sampled_mirror's
                 sample, log_joint and score_gradient
"""
import math

import numpy as np
import torch

import hp_reference as hp
import ksd_sampled_mirror as km
import mps_mirror as mm
import mps_sampled_mirror as sm

LD = sm.LD


def all_bits(n):
    return sm.bits_of_idx(np.arange(1 << n, dtype=np.int64), n)


def score_rows(cores, bits, env=None, dtype=None):
    """dict rows, rows_abs [n, 2 D^2, B], mu, mu_abs [n, 2, D, D], psi, psi_abs [B], kappa [B] (psi_abs / |psi|), q [B]
    (psi^2 / Z).  A sample with psi = 0 gets an all-zero column."""
    dtype = dtype or LD
    cores = np.asarray(cores, dtype=np.float64)
    n, _, D, _ = cores.shape
    env = env or sm.environments(cores, dtype)
    A, Aa = cores.astype(dtype), np.abs(cores).astype(dtype)
    L, R = mm._left_right(A, bits, dtype)
    La, Ra = mm._left_right(Aa, bits, dtype)
    psi, psia = L[n][:, 0], La[n][:, 0]
    ok = psi != 0
    safe = np.where(ok, psi, 1)
    B = bits.shape[0]
    rows = np.zeros((n, 2, D, D, B), dtype)
    rows_abs = np.zeros((n, 2, D, D, B), dtype)
    mu = np.zeros((n, 2, D, D), dtype)
    mua = np.zeros((n, 2, D, D), dtype)
    two = dtype(2)
    for k in range(1, n + 1):
        for s in (0, 1):
            mu[k - 1, s] = two * (env["L"][k - 1] @ A[k - 1, s] @ env["E"][k]) / env["Z"]
            mua[k - 1, s] = two * (env["L_abs"][k - 1] @ Aa[k - 1, s] @ env["E_abs"][k]) / env["Z"]
            on = (bits[:, k - 1] == s) & ok
            t = two * np.einsum('ba,bc->acb', L[k - 1] * (on / safe)[:, None], R[k])
            ta = two * np.einsum('ba,bc->acb', La[k - 1] * (on / np.abs(safe))[:, None], Ra[k])
            rows[k - 1, s] = np.where(ok[None, None, :], t - mu[k - 1, s][:, :, None], 0)
            rows_abs[k - 1, s] = np.where(ok[None, None, :], ta + mua[k - 1, s][:, :, None], 0)
    return {"rows": rows.reshape(n, 2 * D * D, B), "rows_abs": rows_abs.reshape(n, 2 * D * D, B), "mu": mu, "mu_abs": mua,
            "psi": psi, "psi_abs": psia, "kappa": np.where(ok, psia / np.abs(safe), np.inf), "q": psi * psi / env["Z"]}


def fisher(rows, B=None, rows_abs=None):
    """dict site [n, R, R], full [P, P] = rows rows^T / B, and site_abs / full_abs = |rows| |rows|^T / B (from rows_abs
    where given: then the products of the absolute-term values)."""
    n, R, Bn = rows.shape
    B = Bn if B is None else B
    ra = np.abs(rows) if rows_abs is None else rows_abs
    X, Xa = rows.reshape(n * R, Bn), ra.reshape(n * R, Bn)
    den = rows.dtype.type(B)
    full, fulla = X @ X.T / den, Xa @ Xa.T / den
    site = np.stack([full[k * R:(k + 1) * R, k * R:(k + 1) * R] for k in range(n)])
    sitea = np.stack([fulla[k * R:(k + 1) * R, k * R:(k + 1) * R] for k in range(n)])
    return {"site": site, "full": full, "site_abs": sitea, "full_abs": fulla}


def exact_fisher(cores, dtype=None):
    """[P, P]: sum_z q_z o_z o_z^T over all outcomes, and the rows' dict (q among its entries)."""
    dtype = dtype or LD
    n = np.asarray(cores).shape[0]
    sr = score_rows(cores, all_bits(n), dtype=dtype)
    X = sr["rows"].reshape(-1, 1 << n)
    return (X * sr["q"][None, :]) @ X.T, sr


def damped_solve(F, g, damping):
    """x with (F + damping I) x = g by Cholesky (lower, row by row) in F's own arithmetic, or None when a pivot is not
    positive and finite."""
    P = F.shape[0]
    dt = F.dtype.type
    W = np.array(F, copy=True)
    W[np.arange(P), np.arange(P)] += dt(damping)
    Lc = np.zeros_like(W)
    for j in range(P):
        piv = W[j, j] - Lc[j, :j] @ Lc[j, :j]
        if not (piv > 0) or not np.isfinite(piv):
            return None
        Lc[j, j] = np.sqrt(piv)
        if j + 1 < P:
            Lc[j + 1:, j] = (W[j + 1:, j] - Lc[j + 1:, :j] @ Lc[j, :j]) / Lc[j, j]
    y = np.zeros(P, W.dtype)
    for j in range(P):
        y[j] = (g[j] - Lc[j, :j] @ y[:j]) / Lc[j, j]
    x = np.zeros(P, W.dtype)
    for j in range(P - 1, -1, -1):
        x[j] = (y[j] - Lc[j + 1:, j] @ x[j + 1:]) / Lc[j, j]
    return x


def precondition(cores, bits, grad, damping, blocks="site", dtype=None):
    """(delta [n, 2, D, D], info [nblocks] of 0 / 1) in the mirror's arithmetic."""
    dtype = dtype or LD
    cores = np.asarray(cores, dtype=np.float64)
    n, _, D, _ = cores.shape
    R = 2 * D * D
    F = fisher(score_rows(cores, bits, dtype=dtype)["rows"])
    g = np.asarray(grad).astype(dtype)
    if blocks == "full":
        x = damped_solve(F["full"], g.reshape(-1), damping)
        return (g if x is None else x).reshape(cores.shape), np.array([int(x is None)])
    out, info = np.zeros((n, R), dtype), np.zeros(n, np.int64)
    for k in range(n):
        x = damped_solve(F["site"][k], g.reshape(n, R)[k], damping)
        out[k], info[k] = (g.reshape(n, R)[k] if x is None else x), int(x is None)
    return out.reshape(cores.shape), info


def epoch_weights(kind, packed, s, n, B, p_floor=1e-30, length_scale=1.0):
    """(loss, w [B]) of one epoch in float64 from the draws s (mps_sampled_mirror.sample): the ELBO trainer's or the KSD
    trainer's ('ksd2' objective)."""
    if kind == "elbo":
        f = np.asarray(s["logq"], dtype=np.float64) - sm.log_joint(packed, s["bits"], p_floor)
        loss = f.mean()
        return float(loss), (f - loss) / (B - 1)
    S, _, _ = km.scores(packed, s["idx"], n, p_floor, X=km.F64)
    K, _, _ = km.kappa_bound(s["idx"], S, n, length_scale, X=km.F64)
    r, T = km.rowsums(K)
    U, _, w = km.weights(r, T, B)
    return float(U), np.asarray(w, dtype=np.float64)


def replay(kind, cores0, packed, B, seed, epochs, lr, damping, blocks="site", momentum=0.0, clip=10.0, p_floor=1e-30,
           margin=1e-8, length_scale=1.0):
    """The sampled trainers' train(optimizer_type='sgd', sgd_momentum=momentum, natural_gradient=...) on the CPU in float64:
    dict loss, grad_norm (of the preconditioned step, before the clip), natgrad_info per epoch, idx of every epoch, the final
    cores and `undecided`.  damping None: the plain gradient."""
    cores = torch.nn.Parameter(torch.as_tensor(np.asarray(cores0), dtype=torch.float64).clone())
    n = cores.shape[0]
    opt = torch.optim.SGD([cores], lr=lr, momentum=momentum)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=epochs, eta_min=lr / 10)
    hist = {"loss": [], "grad_norm": [], "natgrad_info": [], "idx": [], "undecided": 0}
    for ep in range(epochs):
        opt.zero_grad()
        c = cores.detach().numpy()
        s = sm.sample(c, seed, ep, B, dtype=np.float64, margin=margin)
        hist["undecided"] += s["undecided"]
        loss, w = epoch_weights(kind, packed, s, n, B, p_floor, length_scale)
        g = sm.score_gradient(c, s["bits"], w, dtype=np.float64)["grad"]
        info = np.zeros(0, np.int64)
        if damping is not None:
            g, info = precondition(c, s["bits"], g, damping, blocks, dtype=np.float64)
        cores.grad = torch.as_tensor(np.ascontiguousarray(g, dtype=np.float64))
        gn = torch.nn.utils.clip_grad_norm_([cores], clip)
        opt.step()
        sched.step()
        hist["loss"].append(loss)
        hist["grad_norm"].append(float(gn))
        hist["natgrad_info"].append(int((info != 0).sum()))
        hist["idx"].append(s["idx"])
    hist["cores"] = cores.detach().numpy().copy()
    return hist


# ---------------------------------------------------------------------------------------------- the kernels' error bounds
def c_rows(n, D, kappa_b, kappa_Z):
    """Derived C of one score-row entry of bornvi_mps_score_rows, units of EPS64 on the entry's absolute-term value
    (rows_abs), every rounding a whole unit, derived as test_gpu_mps_sampled_kernel.py derives C_SCORE:
      the sample term 2 l[a] r[c] / psi: l_{k-1} and r_k are (n - 1) D-term fma chains together, 1 / psi_b costs
        C_PSI kappa_b = (n D + 2) kappa_b, then the quotient 2 / r0 and the two products: 3;
      mu: L_{k-1} and E_k (C_ENV(n - 1) = (n - 1)(3 D + 1) together), the two D-term chains (2 D), 1 / Z
        (C_ENV(n) kappa_Z), the quotient and the doubling: 2;
      the subtraction: 1.
    Both terms are bounded by the same rows_abs entry, so the constant is 1 + the larger of the two."""
    sample = (n - 1) * D + (n * D + 2) * np.asarray(kappa_b, dtype=np.float64) + 3
    mu = (n - 1) * (3 * D + 1) + 2 * D + n * (3 * D + 1) * kappa_Z + 2
    return 1.0 + np.maximum(sample, mu)


def c_gram(ld):
    """Derived C of one Gram entry of bornvi_score_fisher_gram, units of EPS64 on sum_b |o_a| |o_b| / B of the rows it was
    given: the SYRK chain over ld columns (hp_reference.syrk_geometry: at most `slab` additions inside a slab's MFMAs, the
    per_wg slab results and the G partials in order), every rounding a whole unit, and the one division by B."""
    return float(sum(hp.syrk_geometry(ld)) + 1)
