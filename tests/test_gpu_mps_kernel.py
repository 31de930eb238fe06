"""bornvi_mps_probs / bornvi_mps_vjp against the per-z extended-precision mirror (mps_mirror.reference), per entry the
hp_reference.ratio way, and their contract: exact zeros, bitwise reproducible, optional outputs, refused sizes, capturable.

Shapes.  The kernels change path at these sizes (kernels_mps.hip): levels k <= 10 and, for n <= 11, the last level run in
one workgroup (one partial of Z and of every dA_k), n >= 12 streams the levels above 10, one launch each, with several
workgroups (n = 12: 4 and 8 of them; up to 2^18 parents a workgroup takes 256 of them, from 2^19 parents on, which is
level 20 and so n = 20, more than 256);
the elementwise passes over 2^n use one workgroup up to n = 12 and several from n = 13.  The issue's list n in {1, 2, 3, 5,
9, 12, 13} lies on both sides of the second boundary; n = 11 is added for the other side of the first.

Error bounds, derived from the kernels' operation chains (units of EPS64 = 2^-52; every rounding is counted as a whole
unit, twice what a correctly rounded operation can do, as hp_reference.dense_constants does):
  psi: n levels, each a D-term fma chain:  |err| <= C_PSI eps psi_abs,  C_PSI = n D + 2.
  Z = sum psi^2: a term psi^2 errs by (2 C_PSI + 1) eps |psi| psi_abs; the sum is a chain of T1 = 2 x (parents per thread)
    fmas, 6 butterfly levels, 4 wave totals, then the partials the same way (T2 = partials per thread + 10):
    |err| <= eps [(2 C_PSI + 1) S + T_Z Z],  S = sum |psi| psi_abs,  T_Z = T1 + 10 + T2.
  q = psi^2 / Z: the square and the quotient (2), the term's own error and Z's relative error:
    |err| <= eps { [(2 C_PSI + 1) |psi| psi_abs + 2 psi^2] / Z + q [(2 C_PSI + 1) S / Z + T_Z] };   sum q: that, summed.
  grad_cores against grad_abs: C_GRAD = C_GAMMA + max over k of the chain from G_n to dA_k, with kappa = Z_abs / Z >= S / Z:
    c = sum q g: q relative to q_abs = psi_abs^2 / Z by C_Q = 2 C_PSI + 3 + (2 C_PSI + 1) kappa + T_Z, the fma and the tree T_C;
    gamma = 2 psi (g - c) / Z: psi (C_PSI), the difference (1, and c's error C_Q + T_C), the product, the quotient and
      Z's relative error:  C_GAMMA = C_PSI + C_Q + T_C + 3 + (2 C_PSI + 1) kappa + T_Z;
    G_{j-1} from G_j: two D-term chains and their sum: D + 1 per level, n - k levels down to G_k;
    V_{k-1}: (k - 1) D;  a product V G and its sum over p: the MFMA adds the parents of a wave in order (W_k of them),
      3 additions join the waves, the finishing launch adds ceil(workgroups / 4) partials in order and 3 more:
    chain(k) = (n - k)(D + 1) + (k - 1) D + 1 + W_k + 3 + ceil(nwg_k / 4) + 3.
The constants are not fitted: each test prints the worst ratio beside its C.
Larger shapes (n = 16, D = 8 and n = 20, D = 4) are held to the same bounds against the float64 doubling mirror, whose own
error obeys the same C_PSI / C_GRAD chains without the tree terms: the bound there is doubled."""
import functools
import math

import numpy as np
import pytest
import torch

import hp_reference as hp
import mps_mirror as mm

pytestmark = pytest.mark.gpu

ALL_N = (1, 2, 3, 5, 9, 11, 12, 13)
ALL_D = (1, 2, 3, 5, 8, 16, 32)
SMALL = sorted(set([(n, 3) for n in ALL_N] + [(5, D) for D in ALL_D] + [(1, 32), (13, 32), (1, 1), (2, 1), (2, 2), (2, 5), (3, 2),
                                                                          (3, 8), (9, 2), (9, 16), (9, 32), (11, 5), (12, 1),
                                                                          (12, 8), (12, 16), (13, 2), (13, 5), (13, 16)]))
LARGE = [(16, 8), (20, 4)]
FUSED, THREADS, MAX_WG, Q_PER_WG = 10, 256, 1024, 4096


def dev():
    return torch.device("cuda", torch.cuda.current_device())


def geometry(n):
    """Per level k = 1 .. n: (workgroups, parents per wave) as kernels_mps.hip splits the work."""
    out = {}
    for k in range(1, n + 1):
        P = 1 << (k - 1)
        fused = k <= FUSED or (k == n and n <= FUSED + 1)
        nwg = 1 if fused else min(MAX_WG, P // THREADS)
        per_wg = P // nwg
        out[k] = (nwg, ((-(-per_wg // 4)) + 3) & ~3)
    return out


def constants(n, D, kappa):
    geo = geometry(n)
    c_psi = n * D + 2
    nwg_n = geo[n][0]
    t1 = 2 * max(1, -(-(1 << (n - 1)) // (nwg_n * THREADS)))
    t_z = t1 + 10 + (-(-nwg_n // THREADS)) + 10
    N = 1 << n
    Gq = min(1024, -(-N // Q_PER_WG))
    t_c = (-(-(-(-N // Gq)) // THREADS)) + 10 + (-(-Gq // THREADS)) + 10 + 1
    c_q = 2 * c_psi + 3 + (2 * c_psi + 1) * kappa + t_z
    c_gamma = c_psi + c_q + t_c + 3 + (2 * c_psi + 1) * kappa + t_z
    chain = max((n - k) * (D + 1) + (k - 1) * D + 1 + geo[k][1] + 3 + (-(-geo[k][0] // 4)) + 3 for k in range(1, n + 1))
    return {"psi": float(c_psi), "t_z": float(t_z), "grad": float(c_gamma + chain)}


def make_inputs(n, D, seed=0):
    gen = torch.Generator().manual_seed(1000 * n + D + seed)
    eye = torch.eye(D, dtype=torch.float64).expand(n, 2, D, D)
    cores = (eye + 0.3 * torch.randn(n, 2, D, D, dtype=torch.float64, generator=gen)) / math.sqrt(2.0)
    g = torch.randn(1 << n, dtype=torch.float64, generator=gen)
    return cores.contiguous(), g


@functools.lru_cache(maxsize=None)
def case(n, D):
    """(cores, g, the mirror's reference) of one shape, computed once and shared by the tests."""
    cores, g = make_inputs(n, D)
    return cores, g, mm.reference(cores.numpy(), g.numpy())


def run(cores, g, want_q32=True, want_psi=True):
    from tensornetworks_amd import backend
    c = cores.to(dev())
    q32, q64, psi, Z = backend.mps_probs(c, want_q32=want_q32, want_psi=want_psi)
    grad = backend.mps_vjp(c, g.to(dev())) if g is not None else None
    torch.cuda.synchronize()
    return q32, q64, psi, Z, grad


def q_bound(ref, C):
    psi, pa, Z = np.abs(ref["psi"]), ref["psi_abs"], ref["Z"]
    S = (psi * pa).sum()
    return ((2 * C["psi"] + 1) * psi * pa + 2 * psi * psi) / Z + ref["q"] * ((2 * C["psi"] + 1) * S / Z + C["t_z"])


def check(n, D, got, ref, scale=1.0):
    q32, q64, psi, Z, grad = got
    C = constants(n, D, float(ref["Z_abs"] / ref["Z"]))
    r_psi, at_psi = hp.worst(hp.ratio(psi.cpu().numpy(), ref["psi"], ref["psi_abs"], X=hp._LongDouble))
    qb = q_bound(ref, C)
    r_q, at_q = hp.worst(hp.ratio(q64.cpu().numpy(), ref["q"], qb, X=hp._LongDouble))
    # (the sum itself is taken in extended precision on the host; 1 unit for rounding it to float64)
    r_sum, _ = hp.worst(hp.ratio(float(q64.cpu().numpy().astype(np.longdouble).sum()), np.longdouble(1), qb.sum() + 1, X=hp._LongDouble))
    r_g, at_g = hp.worst(hp.ratio(grad.cpu().numpy(), ref["grad"], ref["grad_abs"], X=hp._LongDouble))
    print(f"n={n} D={D}: psi {r_psi:.3g} at {at_psi} (C {scale * C['psi']:.0f}); q {r_q:.3g} at {at_q} (C {scale:.0f}); "
          f"sum q {r_sum:.3g} (C {scale:.0f}); grad {r_g:.3g} at {at_g} (C {scale * C['grad']:.0f})")
    assert r_psi <= scale * C["psi"]
    assert r_q <= scale
    assert r_sum <= scale
    assert r_g <= scale * C["grad"]
    return C


@pytest.mark.parametrize("n,D", SMALL)
def test_small_shapes(n, D):
    """psi, q, sum q and grad_cores per entry against extended precision; the exact facts of the contract."""
    cores, g, ref = case(n, D)
    got = run(cores, g)
    check(n, D, got, ref)
    q32, q64, psi, Z, grad = got
    assert torch.equal(q32, q64.float())
    Cc = constants(n, D, 1.0)
    zb = (2 * Cc["psi"] + 1) * (np.abs(ref["psi"]) * ref["psi_abs"]).sum() + Cc["t_z"] * ref["Z"]
    r_z, _ = hp.worst(hp.ratio(float(Z), ref["Z"], zb, X=hp._LongDouble))
    print(f"n={n} D={D}: Z {r_z:.3g} (C 1)")
    assert r_z <= 1.0
    # unused entries: rows a > 0 of the first core, columns b > 0 of the last
    if D > 1:
        assert torch.all(grad[0, :, 1:, :] == 0.0) and torch.all(grad[n - 1, :, :, 1:] == 0.0)
    # bitwise reproducible, and the optional outputs change nothing
    again = run(cores, g)
    assert torch.equal(again[1], q64) and torch.equal(again[4], grad) and torch.equal(again[2], psi)
    bare = run(cores, None, want_q32=False, want_psi=False)
    assert bare[0] is None and bare[2] is None and torch.equal(bare[1], q64)


@pytest.mark.parametrize("n,D", LARGE)
def test_large_shapes(n, D):
    """The streamed levels with many workgroups, against the float64 doubling mirror (bounds doubled: the mirror errs too)."""
    cores, g = make_inputs(n, D)
    val = mm.doubling(cores.numpy(), g.numpy())
    ab = mm.doubling(cores.numpy(), g.numpy(), Z_true=val["Z"])
    ref = {"psi": val["psi"].astype(np.longdouble), "psi_abs": ab["psi"].astype(np.longdouble), "Z": np.longdouble(val["Z"]),
           "Z_abs": np.longdouble((ab["psi"] ** 2).sum()), "q": val["q"].astype(np.longdouble),
           "grad": val["grad"].astype(np.longdouble), "grad_abs": ab["grad"].astype(np.longdouble)}
    got = run(cores, g)
    check(n, D, got, ref, scale=2.0)
    assert torch.equal(got[0], got[1].float())
    assert torch.equal(run(cores, g)[4], got[4])


@pytest.mark.parametrize("n,D", [(5, 3), (9, 5), (12, 8)])
def test_invariances(n, D):
    """Gauge change A_k -> A_k M, A_{k+1} -> M^-1 A_{k+1} leaves q unchanged; <grad_cores[k], cores[k]> = 0 for every k (q does
    not change when one core is scaled).  Both to the derived bounds: the gauged cores' own q bound, and the inner product
    against sum |grad_abs| |cores| with C_GRAD."""
    cores, g, ref = case(n, D)
    got = run(cores, g)
    C = constants(n, D, float(ref["Z_abs"] / ref["Z"]))
    inner = (got[4].cpu().numpy().astype(np.longdouble) * cores.numpy()).sum(axis=(1, 2, 3))
    bound = (ref["grad_abs"] * np.abs(cores.numpy())).sum(axis=(1, 2, 3))
    r_in, at = hp.worst(hp.ratio(hp.to_f64(inner), np.zeros(n, np.longdouble), bound, X=hp._LongDouble))
    print(f"n={n} D={D}: <grad, cores> {r_in:.3g} at {at} (C {C['grad'] + 2 * D * D:.0f})")
    assert r_in <= C["grad"] + 2 * D * D
    if n >= 2:
        gen = torch.Generator().manual_seed(7)
        k = n // 2
        M = torch.eye(D, dtype=torch.float64) + 0.1 * torch.randn(D, D, dtype=torch.float64, generator=gen)
        gauged = cores.clone()
        gauged[k - 1] = cores[k - 1] @ M
        gauged[k] = torch.linalg.solve(M, cores[k])
        ref2 = mm.reference(gauged.numpy())
        q2 = run(gauged, None)[1]
        C2 = constants(n, D, float(ref2["Z_abs"] / ref2["Z"]))
        # q of the gauged cores against the ORIGINAL cores' q: the kernel's bound on the gauged cores plus what rounding the
        # gauged cores themselves moves q by, to first order: the product A M errs by D + 1 units per entry, the solve by
        # D cond(M) + 1, so psi moves by r eps psi_abs with r their sum, and q = psi^2 / Z by 2 |psi| dpsi / Z + q dZ / Z
        r = (D + 1) + (D * float(np.linalg.cond(M.numpy())) + 1)
        p2, pa2, Z2 = np.abs(ref2["psi"]), ref2["psi_abs"], ref2["Z"]
        slack = r * (2 * p2 * pa2 / Z2 + ref2["q"] * 2 * (p2 * pa2).sum() / Z2)
        r_q, at = hp.worst(hp.ratio(q2.cpu().numpy(), ref["q"], q_bound(ref2, C2) + slack, X=hp._LongDouble))
        print(f"n={n} D={D}: gauge q {r_q:.3g} at {at} (C 1)")
        assert r_q <= 1.0


def test_failure_paths():
    """All-zero cores: Z = 0, every q NaN, no error.  n = 27, D = 33 and D = 0 are refused before any launch with
    BORNVI_ERR_UNSUPPORTED (-4)."""
    from tensornetworks_amd import _ext, backend
    q32, q64, psi, Z, grad = run(torch.zeros(4, 2, 3, 3, dtype=torch.float64), torch.ones(16, dtype=torch.float64))
    assert float(Z) == 0.0 and bool(torch.isnan(q64).all()) and bool(torch.isnan(q32).all())
    h = _ext.handle_for(dev())
    lib = _ext.lib()
    buf = torch.zeros(1 << 16, dtype=torch.float64, device=dev())
    for n, D in ((27, 2), (3, 33), (3, 0), (0, 2)):
        assert lib.bornvi_mps_workspace_bytes(h.h, n, D) == 0
        assert lib.bornvi_mps_probs(h.h, n, D, backend._ptr(buf), backend._ptr(buf), None, None, backend._ptr(buf),
                                    backend._ptr(buf), buf.numel() * 8, None) == -4
        assert lib.bornvi_mps_vjp(h.h, n, D, backend._ptr(buf), backend._ptr(buf), backend._ptr(buf), backend._ptr(buf),
                                  buf.numel() * 8, None) == -4
    with pytest.raises(backend.BornviError):
        backend.mps_probs(torch.zeros(3, 2, 33, 33, dtype=torch.float64, device=dev()))
    with pytest.raises(backend.BornviError):
        backend.mps_probs(torch.zeros(27, 2, 1, 1, dtype=torch.float64, device=dev()))


@pytest.mark.parametrize("n,D", [(6, 3), (12, 4)])
def test_capture(n, D):
    """probs + vjp captured once after an eager call; two replays with the cores changed in place equal eager bitwise."""
    from tensornetworks_amd import backend
    cores, g = make_inputs(n, D)
    c, gd = cores.to(dev()), g.to(dev())
    backend.mps_probs(c)
    backend.mps_vjp(c, gd)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        backend.mps_probs(c)          # (the side stream's own workspace, before the capture)
        backend.mps_vjp(c, gd)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        q32, q64, _, Z = backend.mps_probs(c)
        grad = backend.mps_vjp(c, gd)
    for step in (1, 2):
        c.copy_(make_inputs(n, D, seed=step)[0])
        graph.replay()
        torch.cuda.synchronize()
        got = (q64.clone(), q32.clone(), grad.clone())
        e32, e64, _, _ = backend.mps_probs(c)
        egrad = backend.mps_vjp(c, gd)
        torch.cuda.synchronize()
        assert torch.equal(got[0], e64) and torch.equal(got[1], e32) and torch.equal(got[2], egrad)
