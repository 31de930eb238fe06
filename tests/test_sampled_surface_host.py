"""Host checks of the surface the three sampled MPS families share (born_machine_sampled.SampledSurface), no device: the
constructors' parameters bit for bit against tests/golden/sampled_init_parent_bits.npz (recorded before the families moved
onto the shared surface), the structural fact that every shared method is one function object on all three classes, the
refused methods' wording, a sampled trainer that names no machine class, and the real family's backend calls raising the
documented BornviError for a non-tensor epoch or w."""
import ast
import importlib.util
import inspect
import os

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "sampled_init_parent_bits.npz")
# the cases and run() are the recording script's own: what is compared is what was recorded
_spec = importlib.util.spec_from_file_location("make_golden_sampled_init_bits",
                                               os.path.join(HERE, "golden", "make_golden_sampled_init_bits.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)

SHARED = ("sample_indices", "bits_of", "indices_of", "sample", "score_vjp", "get_log_q_z_x", "get_probabilities", "kernel_input",
          "_init_sampled", "_check_enumerated")
CLASS_NAMES = ("SampledMPSBornMachine", "ComplexSampledMPSBornMachine", "PurifiedSampledMPSBornMachine")


def classes():
    from tensornetworks_amd import ComplexSampledMPSBornMachine, PurifiedSampledMPSBornMachine, SampledMPSBornMachine
    return SampledMPSBornMachine, ComplexSampledMPSBornMachine, PurifiedSampledMPSBornMachine


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("case", rec.CASES, ids=rec.case_id)
def test_constructors_give_the_recorded_bits(golden, case):
    got = rec.run(case)
    prefix = rec.case_id(case) + "/"
    assert sorted(prefix + k for k in got) == sorted(k for k in golden if k.startswith(prefix))
    for name, a in got.items():
        want = golden[prefix + name]
        assert a.dtype == want.dtype and a.shape == want.shape and a.tobytes() == want.tobytes(), (rec.case_id(case), name)


def test_shared_methods_are_one_function_object():
    from tensornetworks_amd.born_machine_base import MPSCores
    from tensornetworks_amd.born_machine_sampled import SampledSurface
    real, cx, pur = classes()
    for name in SHARED:
        fn = getattr(SampledSurface, name)
        assert inspect.isfunction(fn), name
        assert all(getattr(cls, name) is fn for cls in (real, cx, pur)), name
    assert real._with_cores.__func__ is cx._with_cores.__func__ is pur._with_cores.__func__ is SampledSurface._with_cores.__func__
    for name in ("environments", "draw", "score_gradient"):          # the three hooks are each family's own
        fns = [getattr(cls, name) for cls in (real, cx, pur)]
        assert len(set(fns)) == 3 and getattr(SampledSurface, name) not in fns, name
    # the two overrides, each stated once
    assert real.log_prob is cx.log_prob is SampledSurface.log_prob and pur.log_prob is not SampledSurface.log_prob
    assert "log_prob" in vars(pur) and "log_prob" not in vars(real) and "log_prob" not in vars(cx)
    assert cx.probabilities64 is pur.probabilities64 is SampledSurface.probabilities64
    assert "probabilities64" in vars(real) and real.probabilities64 is not SampledSurface.probabilities64
    # bond_dim is the purified family's own (cores [n, 2, m, D, D]); the real family keeps MPSCores, the others are not one
    assert "bond_dim" in vars(pur) and pur(3, bond_dim=5, purification_dim=3, init_method="zero").bond_dim == 5
    assert issubclass(real, MPSCores) and not issubclass(cx, MPSCores) and not issubclass(pur, MPSCores)
    assert all(issubclass(cls, torch.nn.Module) for cls in (real, cx, pur)) and not issubclass(SampledSurface, torch.nn.Module)
    from tensornetworks_amd import backend
    assert (real.ENUMERATED_MAX_N, cx.ENUMERATED_MAX_N, pur.ENUMERATED_MAX_N) == (backend.MPS_MAX_N, 20, 20)
    assert (real.NATURAL_GRADIENT, cx.NATURAL_GRADIENT, pur.NATURAL_GRADIENT) == (True, False, False)


def test_refused_methods_name_the_real_family_in_the_familys_own_words():
    real, cx, pur = classes()
    assert set(cx.REFUSED) == set(pur.REFUSED) and len(cx.REFUSED) == 13
    assert not hasattr(real, "REFUSED")
    for cls, word in ((cx, "complex cores"), (pur, "purified cores")):
        bm = cls(3, bond_dim=2, init_method="zero")
        for name in cls.REFUSED:
            assert callable(getattr(real, name)) and getattr(cls, name) is not getattr(real, name)
            with pytest.raises(ValueError, match="SampledMPSBornMachine") as e:
                getattr(bm, name)()
            assert word in str(e.value) and name in str(e.value)
            assert getattr(cls, name).__name__ == name and word in getattr(cls, name).__doc__


def test_trainer_names_no_machine_class():
    from tensornetworks_amd import sampled_trainer
    tree = ast.parse(inspect.getsource(sampled_trainer))
    for node in ast.walk(tree):
        if isinstance(node, ast.Call) and isinstance(node.func, ast.Name) and node.func.id == "isinstance" and len(node.args) == 2:
            named = {n.id for n in ast.walk(node.args[1]) if isinstance(n, ast.Name)} | \
                    {n.attr for n in ast.walk(node.args[1]) if isinstance(n, ast.Attribute)}
            assert not named & set(CLASS_NAMES), ast.unparse(node)
    real, cx, pur = classes()
    assert {k: v[0] for k, v in sampled_trainer.FAMILIES.items()} == {"real": real, "complex": cx, "purified": pur}
    assert {k: v[1] for k, v in sampled_trainer.FAMILIES.items()} == {"real": (), "complex": (), "purified": ("purification_dim",)}


def test_real_backend_calls_raise_the_documented_error():
    from tensornetworks_amd import backend
    from tensornetworks_amd._ext import BornviError
    c = torch.zeros(4, 2, 2, 2, dtype=torch.float64)
    idx = torch.zeros(5, dtype=torch.int64)
    with pytest.raises(BornviError, match="epoch"):
        backend.mps_sample(c, 8, 0, 3)
    with pytest.raises(BornviError, match="w: expected"):
        backend.mps_score_vjp(c, idx, [1.0] * 5)
    with pytest.raises(BornviError, match="w: expected"):
        backend.mps_score_vjp(c, idx, None)
