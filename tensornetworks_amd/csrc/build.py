#!/usr/bin/env python3
"""Builds libbornvi_hip.so for gfx950 (MI355X) with hipcc; in-tree output next to the package.
One object per source file (compiled in parallel, rebuilt only when the file or a header changed), then one link."""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.dirname(HERE)
REPO = os.path.dirname(PKG)
SOURCES = ["api.hip", "kernels_circuit.hip", "kernels_circuit8.hip", "kernels_stein.hip", "kernels_batched.hip", "kernels_adjoint.hip", "kernels_shots.hip", "kernels_born_table.hip", "kernels_reinforce.hip", "kernels_elbo.hip", "kernels_fisher.hip", "kernels_qfi.hip", "kernels_mps.hip", "kernels_mps_sample.hip", "kernels_mps_sample_gram.hip", "kernels_mps_query.hip", "kernels_mps_canon.hip", "kernels_mps_twosite.hip", "kernels_cmps.hip", "kernels_lps.hip", "kernels_ttn.hip", "kernels_mmd.hip", "kernels_ksd_sampled.hip", "kernels_cg.hip", "plan.cpp"]
HEADERS = [os.path.join(HERE, h) for h in ("plan.hpp", "kernels.hpp", "circuit_dev.hpp", "philox_dev.hpp", "shots_dev.hpp", "mps_sample_dev.hpp", "mps_canon_dev.hpp", "syrk_f64.hpp", "reduce_dev.hpp", "ttn_dev.hpp", "exports.map")] + [os.path.join(REPO, "include", h) for h in ("bornvi.h", "bornvi_twosite.h", "bornvi_cmps.h", "bornvi_mmd.h", "bornvi_lps.h", "bornvi_ttn.h")]
OUT = os.path.join(PKG, "libbornvi_hip.so")
OBJ = os.path.join(HERE, "_obj")
FLAGS = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC", "-fvisibility=hidden", "-I" + os.path.join(REPO, "include"), "-I" + HERE,
         "-Rpass-analysis=kernel-resource-usage"]

# Register-allocation guard rails.  The hot kernels sit a few registers below a cliff: a small source edit has more than
# once made the compiler spill hundreds of VGPRs to scratch (the symmetric contraction went from 2.6 to 6.6 ms that way,
# with identical results), and in the circuit engine a scratch access inside the tile loop would also break the
# hand-counted vmcnt waits.  The build fails when a kernel leaves its budget: (max scratch bytes per lane, max VGPR spills).
RESOURCE_BUDGET = {
    "quadform_sym_kernel": (0, 0),
    "quadform_batched_kernel": (0, 0),
    "quadform_kernel": (0, 0),
    "gram_tables_kernel": (0, 0),                 # the Gram builder: up to 163 VGPRs (n = 16), no scratch
    "circuit_pass_fast_kernelILb": (0, 0),        # 16 amplitudes per thread, both instantiations: no scratch
    "circuit_pass_r3_kernelILb0": (0, 0),         # 8 amplitudes per thread: <= 128 VGPRs (four waves per SIMD) without scratch
    "shots_mass_kernel": (0, 0),                  # finite-shot sampler (kernels_shots.hip): no scratch anywhere
    "shots_draw_kernel": (0, 0),
    "born_table_stats_kernel": (0, 0),            # classical Born machine (kernels_born_table.hip): no scratch anywhere
    "born_table_probs_kernel": (0, 0),
    "born_table_entropy_kernel": (0, 0),
    "born_table_vjp_stats_kernel": (0, 0),
    "born_table_vjp_kernel": (0, 0),
    "reinforce_stats_kernel": (0, 0),             # REINFORCE step of the classical adversarial trainer (kernels_reinforce.hip)
    "reinforce_scatter_kernel": (0, 0),
    "reinforce_finish_kernel": (0, 0),
    "reinforce_loss_kernel": (0, 0),
    "elbo_weights_kernel": (0, 0),                # exact ELBO (kernels_elbo.hip): no scratch anywhere
    "elbo_finish_kernel": (0, 0),
    "fisher_gram_kernel": (0, 0),                 # natural gradient (kernels_fisher.hip): no scratch anywhere
    "fisher_finish_kernel": (0, 0),
    "spd_solve_kernel": (0, 0),                   # both instantiations: the single solve and one workgroup per system
    "score_gram_kernel": (0, 0),                  # Gram of the score rows: the Fisher kernel's tile with a plain row source
    "score_gram_finish_kernel": (0, 0),
    "qfi_gram_kernel": (0, 0),                    # quantum natural gradient (kernels_qfi.hip): no scratch anywhere
    "qfi_finish_kernel": (0, 0),
    "state_tail_kernel": (0, 0),
    "mps_fwd_fused_kernel": (0, 0),               # MPS Born machine (kernels_mps.hip), every bond-size instantiation: a row of
    "mps_fwd_level_kernel": (0, 0),               # up to 32 doubles per lane lives in registers, no scratch anywhere
    "mps_psi_kernel": (0, 0),
    "mps_q_kernel": (0, 0),
    "mps_gstats_kernel": (0, 0),
    "mps_bwd_fused_kernel": (0, 0),
    "mps_bwd_level_kernel": (0, 0),
    "mps_finish_kernel": (0, 0),
    "mps_env_kernel": (0, 0),                     # sampled MPS (kernels_mps_sample.hip): l, u_0, u_1 (3 x 32 doubles) in registers
    "mps_sample_kernel": (0, 0),
    "mps_score_kernel": (0, 0),
    "mps_score_finish_kernel": (0, 0),
    "mps_score_mu_kernel": (0, 0),                # score rows of the sampled Fisher estimate: l in registers, l and r of the
    "mps_score_rows_kernel": (0, 0),              # site through LDS, no scratch
    "mps_gram_vectors_kernel": (0, 0),            # sample-space Gram (kernels_mps_sample_gram.hip): l, r of the site and the
    "mps_gram_mu_norm_kernel": (0, 0),            # next l (3 x 32 doubles) in registers; the Gram's 2 x 2 fragments of
    "mps_sample_gram_kernel": (0, 0),             # accumulators and the 16 xor-ed index words likewise, no scratch
    "mps_jvp_dot_kernel": (0, 0),                 # matrix-free natural gradient: the tangent sweep holds l, dl and their two
    "mps_score_jvp_kernel": (0, 0),               # products (4 x 32 doubles, 256 of a lone wave's 512 VGPRs), no scratch
    "mps_query_env_kernel": (0, 0),               # posterior queries (kernels_mps_query.hip): the environment step's and the
    "mps_query_logm_kernel": (0, 0),              # sampler's own code, so their budgets
    "mps_sample_clamped_kernel": (0, 0),
    "mps_marginals_kernel": (0, 0),
    "mps_logm_vjp_kernel": (0, 0),                # gradient of log-marginals: the environment step's code in both directions
    "mps_logm_vjp_finish_kernel": (0, 0),
    "mps_canon_kernel": (0, 0),                   # canonical form (kernels_mps_canon.hip): everything lives in LDS, no per-lane arrays
    "mts_init_kernel": (0, 0),                    # two-site sweeps (kernels_mps_twosite.hip): l and r of a sample (2 x 16 doubles)
    "mts_right_kernel": (0, 0),                   # and the four blocks' accumulators in registers; the bond kernel lives in
    "mts_advance_kernel": (0, 0),                 # LDS like the canonicaliser, no scratch
    "mts_accum_kernel": (0, 0),
    "mts_bond_kernel": (0, 0),
    "cmps_env_kernel": (0, 0),                    # complex sampled MPS (kernels_cmps.hip): l, u_0, u_1 (3 x 16 complex) in registers,
    "cmps_sample_kernel": (0, 0),                 # the score kernel's l, r and next vector likewise and four accumulator
    "cmps_score_kernel": (0, 0),                  # fragments; no scratch in any bond-size instantiation
    "cmps_score_finish_kernel": (0, 0),
    "lps_env_kernel": (0, 0),                     # locally purified MPS (kernels_lps.hip): the sampler keeps l and one u (2 x 16
    "lps_sample_kernel": (0, 0),                  # doubles) in registers; a wave of the score kernel a density, its operands and 2 m gradient
    "lps_score_kernel": (0, 0),                   # tiles (4 doubles each); no scratch in any instantiation
    "lps_score_finish_kernel": (0, 0),
    "ttn_env_kernel": (0, 0),                     # tree tensor network (kernels_ttn.hip): the sampler keeps a density and one row's
    "ttn_sample_kernel": (0, 0),                  # products (2 x 64 doubles at D = 8) in registers, its stack in LDS or the workspace;
    "ttn_score_kernel": (0, 0),                   # the score kernel three vectors and four accumulator tiles; no scratch in any
    "ttn_score_finish_kernel": (0, 0),            # instantiation
    "mmd_pass_kernel": (0, 0),                    # MMD (kernels_mmd.hip): a tile's 16 doubles per thread and a radix-16 round in
    "mmd_finish_kernel": (0, 0),                  # registers, the tile and the pair counts' histogram columns in LDS, no scratch
    "hamming_pairs_kernel": (0, 0),
    "hamming_pairs_finish_kernel": (0, 0),
    "hamming_pairs_total_kernel": (0, 0),
    "bn_sample_kernel": (0, 0),                   # ancestral draws from the network: the node values are one 64-bit register
    "cg_init_kernel": (0, 0),                     # the CG recurrence (kernels_cg.hip)
    "cg_step_kernel": (0, 0),
    "cg_finish_kernel": (0, 0),
    "bn_logjoint_kernel": (0, 0),
    "bn_score_samples_kernel": (0, 0),            # sampled KSD (kernels_ksd_sampled.hip): the row side's A fragments (up to 48
    "stein_pairs_prep_kernel": (0, 0),            # doubles per lane) and the tile in flight live in registers, no scratch
    "stein_pairs_kernel": (0, 0),
    "stein_pairs_finish_kernel": (0, 0),
    "circuit_pass_r3_kernelILb1": (0, 0),         # its fused-dot instantiation (last pass only): 8 weights more per thread, exactly
                                                  # 128 VGPRs; a scratch reload is a vector-memory load, and its wait is a wait for the
                                                  # whole prefetched tile (vmcnt retires in issue order)
}


def _stale(target, deps):
    return not os.path.exists(target) or any(os.path.getmtime(target) < os.path.getmtime(d) for d in deps)


def build(force=False, verbose=True):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    srcs = [os.path.join(HERE, s) for s in SOURCES if os.path.exists(os.path.join(HERE, s))]
    os.makedirs(OBJ, exist_ok=True)
    objs, jobs = [], []
    for s in srcs:
        o = os.path.join(OBJ, os.path.basename(s) + ".o")
        objs.append(o)
        if force or _stale(o, [s] + HEADERS + [os.path.abspath(__file__)]):
            jobs.append([hipcc] + FLAGS + ["-c", s, "-o", o])
    if not force and not _stale(OUT, srcs + HEADERS):     # (the objects do not travel to the GPU box; the .so does)
        if verbose:
            print(f"[bornvi] {OUT} is up to date")
        return OUT
    if not os.path.exists(hipcc):
        raise RuntimeError(f"{hipcc} not found and {OUT} is out of date")

    def run(cmd):
        if verbose:
            print("[bornvi]", " ".join(c for c in cmd if not c.startswith("-Rpass")), flush=True)
        if "-c" in cmd:          # keep the compiler's resource remarks next to the object
            r = subprocess.run(cmd, stderr=subprocess.PIPE, text=True)
            with open(cmd[cmd.index("-o") + 1] + ".remarks", "w") as f:
                f.write(r.stderr)
            if r.returncode != 0:
                sys.stderr.write("\n".join(l for l in r.stderr.splitlines() if "remark:" not in l and not l.startswith(" ")) + "\n")
                raise subprocess.CalledProcessError(r.returncode, cmd)
        else:
            subprocess.run(cmd, check=True)
    with ThreadPoolExecutor(max_workers=4) as ex:
        list(ex.map(run, jobs))
    check_resources(objs, verbose)
    run([hipcc, "-shared", "-fPIC", "--offload-arch=gfx950", "-Wl,--version-script=" + os.path.join(HERE, "exports.map"), "-o", OUT] + objs)
    return OUT


def kernel_resources(objs):
    """{mangled kernel name: {"scratch": bytes per lane, "vgpr_spill": n, "vgprs": n, "agprs": n, "sgpr_spill": n}} from
    the remarks files written beside the objects."""
    import re
    out = {}
    for o in objs:
        path = o + ".remarks"
        if not os.path.exists(path):
            continue
        cur = None
        for line in open(path):
            m = re.search(r"remark: Function Name: (\S+)", line)
            if m:
                cur = out.setdefault(m.group(1), {})
                continue
            if cur is None:
                continue
            for key, pat in (("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"), ("vgpr_spill", r"VGPRs Spill: (\d+)"),
                             ("sgpr_spill", r"SGPRs Spill: (\d+)"), ("vgprs", r" VGPRs: (\d+)"), ("agprs", r"AGPRs: (\d+)")):
                m = re.search(pat, line)
                if m:
                    cur[key] = int(m.group(1))
    return out


def check_resources(objs=None, verbose=True):
    if objs is None:
        objs = [os.path.join(OBJ, s + ".o") for s in SOURCES]
    res = kernel_resources(objs)
    problems = []
    for pat, (max_scratch, max_spill) in RESOURCE_BUDGET.items():
        hits = {k: v for k, v in res.items() if pat in k}
        if not hits and res:
            problems.append(f"no kernel matching {pat} in the compiler remarks")
        for k, v in hits.items():
            if v.get("scratch", 0) > max_scratch or v.get("vgpr_spill", 0) > max_spill:
                problems.append(f"{k}: scratch {v.get('scratch')} B/lane (budget {max_scratch}), VGPR spills {v.get('vgpr_spill')} (budget {max_spill})")
            elif verbose:
                print(f"[bornvi] resources ok: {pat}: {v.get('vgprs')} VGPRs + {v.get('agprs')} AGPRs, scratch {v.get('scratch')} B/lane")
    if problems:
        raise RuntimeError("kernel register budget exceeded:\n  " + "\n  ".join(problems))
    return res


if __name__ == "__main__":
    build(force="--force" in sys.argv)
