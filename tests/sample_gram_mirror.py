"""Oracle of the sample-space natural gradient of the sampled MPS Born machine (test infrastructure on
sampled_fisher_mirror, plain NumPy / CPU torch, not under test).  With O [B, P] the centred score rows (fm.score_rows),

  (O^T O / B + damping I)^-1 O^T w = O^T u,   (T + damping I) u = w,   T = O O^T / B.

  sample_gram    T and T_abs [B, B] from score_rows' `rows` / `rows_abs`
  precondition   the dual: delta [n, 2, D, D] = O^T u and info [1] (1: the Cholesky of T + damping I failed, delta = O^T w)
  replay         sampled_fisher_mirror.replay with the dual step in place of the primal one
  c_sample_gram  the derived error constant of one entry of bornvi_mps_score_sample_gram
"""
import numpy as np
import torch

import mps_sampled_mirror as sm
import sampled_fisher_mirror as fm

LD = sm.LD


def sample_gram(cores, bits, env=None, dtype=None, sr=None):
    """dict T, T_abs [B, B] (rows^T rows / B and rows_abs^T rows_abs / B) and the rows' dict `sr`."""
    dtype = dtype or LD
    sr = sr or fm.score_rows(cores, bits, env, dtype=dtype)
    n, R, B = sr["rows"].shape
    X, Xa = sr["rows"].reshape(n * R, B), sr["rows_abs"].reshape(n * R, B)
    den = X.dtype.type(B)
    return {"T": X.T @ X / den, "T_abs": Xa.T @ Xa / den, "sr": sr}


def precondition(cores, bits, w, damping, dtype=None):
    """(delta [n, 2, D, D], info [1] of 0 / 1) by the sample-space solve in the mirror's arithmetic."""
    dtype = dtype or LD
    cores = np.asarray(cores, dtype=np.float64)
    G = sample_gram(cores, bits, dtype=dtype)
    X = G["sr"]["rows"].reshape(-1, bits.shape[0])               # [P, B] = O^T
    wl = np.asarray(w, dtype=np.float64).astype(dtype)
    u = fm.damped_solve(G["T"], wl, damping)
    return (X @ (wl if u is None else u)).reshape(cores.shape), np.array([int(u is None)])


def replay(kind, cores0, packed, B, seed, epochs, lr, damping, momentum=0.0, clip=10.0, p_floor=1e-30, margin=1e-8,
           length_scale=1.0):
    """sampled_fisher_mirror.replay (float64, SGD) with natural_gradient='sample': the same dict."""
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
        loss, w = fm.epoch_weights(kind, packed, s, n, B, p_floor, length_scale)
        g, info = precondition(c, s["bits"], w, damping, dtype=np.float64)
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


# ---------------------------------------------------------------------------------------------- the kernel's error bound
def c_mu(n, D, kappa_Z):
    """One entry of mu in units of EPS64 on mu_abs: the mu branch of sampled_fisher_mirror.c_rows."""
    return (n - 1) * (3 * D + 1) + 2 * D + n * (3 * D + 1) * kappa_Z + 2


def c_sample_gram(n, D, kappa_b, kappa_b2, kappa_Z):
    """Derived C of one entry of bornvi_mps_score_sample_gram, units of EPS64 on T_abs = rows_abs^T rows_abs / B, every
    rounding a whole unit, derived as sampled_fisher_mirror.c_rows and c_gram are.  rows_abs = t_abs + mu_abs entry by
    entry, so B T_abs is the sum of the four products t_abs . t_abs', t_abs . mu_abs, mu_abs . t_abs', mu_abs . mu_abs, and
    each of the kernel's four terms is bounded by its own product: the constant is the largest of the four, plus the three
    additions that combine them (every partial sum is below the sum of the four products) and the division by B.
      sum_k [z = z'] (x . x')(r . r'): x^_bk = cf l^_{k-1} is a (k - 1) D-term chain, 1 / psi_b ((n D + 2) kappa_b, c_rows'
        C_PSI), the quotient 2 / r0 and the product with cf: 2; r^_bk is an (n - k) D-term chain; both samples:
        2 (n - 1) D + (n D + 2)(kappa_b + kappa_b') + 4.  The two dot chains over D4 = D rounded up to 4 terms: 2 D4.
        The product and the n-term sum are one fma per site: n.
      m_b: x^ and r^ of sample b, (n - 1) D + (n D + 2) kappa_b + 2, their product 1, mu's entry c_mu, the D^2-term fma
        chain of a site D^2, the n-term sum n.  m_b' likewise.
      M = sum mu^2: 2 c_mu, the lane's chain of ceil(2 n D^2 / 256) terms, the 6 butterfly steps and the 3 additions of the
        waves."""
    kb, kb2 = np.asarray(kappa_b, dtype=np.float64), np.asarray(kappa_b2, dtype=np.float64)
    D4 = (D + 3) // 4 * 4
    cm = c_mu(n, D, kappa_Z)
    pair = 2 * (n - 1) * D + (n * D + 2) * (kb + kb2) + 4 + 2 * D4 + n
    m1 = (n - 1) * D + (n * D + 2) * kb + 3 + cm + D * D + n
    m2 = (n - 1) * D + (n * D + 2) * kb2 + 3 + cm + D * D + n
    M = 2 * cm + -(-2 * n * D * D // 256) + 9
    return np.maximum(np.maximum(pair, M), np.maximum(m1, m2)) + 4.0
