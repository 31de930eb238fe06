"""tensornetworks_amd -- MI355X-native KSD variational inference with a quantum Born machine.

Drop-in for the hot path of sozoluffy/TensorNetworks (QuantumBornMachine, KSDVariationalInference,
stein_utils) on a hand-written HIP backend (libbornvi_hip.so, C ABI in include/bornvi.h).
"""
from .utils import generate_all_binary_outcomes, calculate_tvd  # noqa: F401

__all__ = ["QuantumBornMachine", "KSDVariationalInference", "ClassicalBornMachine", "MPSBornMachine", "ClassicalKSDVariationalInference",
           "ClassicalAdversarialVariationalInference", "ELBOVariationalInference", "ClassicalELBOVariationalInference",
           "SampledMPSBornMachine", "ComplexSampledMPSBornMachine", "PurifiedSampledMPSBornMachine", "TreeSampledBornMachine",
           "SampledELBOVariationalInference", "SampledKSDVariationalInference",
           "SampledFisherPreconditioner", "SampleSpaceFisherPreconditioner", "CGFisherPreconditioner",
           "AmortisedMPSInference", "HammingMixtureKernel", "MMDObjective", "QuantumMMDTrainer", "ClassicalMMDTrainer",
           "SampledMMDTrainer", "generate_all_binary_outcomes", "calculate_tvd"]


def __getattr__(name):
    if name == "QuantumBornMachine":
        from .quantum_born_machine import QuantumBornMachine
        return QuantumBornMachine
    if name == "KSDVariationalInference":
        from .ksd_vi_quantum import KSDVariationalInference
        return KSDVariationalInference
    if name == "ClassicalBornMachine":
        from .born_machine_classical_sim import ClassicalBornMachine
        return ClassicalBornMachine
    if name == "MPSBornMachine":
        from .born_machine_mps import MPSBornMachine
        return MPSBornMachine
    if name == "ClassicalKSDVariationalInference":      # (the reference's ksd_vi.KSDVariationalInference)
        from .ksd_vi import KSDVariationalInference
        return KSDVariationalInference
    if name == "ClassicalAdversarialVariationalInference":      # (the reference's adversarial_vi.AdversarialVariationalInference)
        from .adversarial_vi_classical import AdversarialVariationalInference
        return AdversarialVariationalInference
    if name == "ELBOVariationalInference":
        from .elbo_vi_quantum import ELBOVariationalInference
        return ELBOVariationalInference
    if name == "ClassicalELBOVariationalInference":
        from .elbo_vi import ELBOVariationalInference
        return ELBOVariationalInference
    if name == "SampledMPSBornMachine":
        from .born_machine_mps_sampled import SampledMPSBornMachine
        return SampledMPSBornMachine
    if name == "ComplexSampledMPSBornMachine":
        from .born_machine_cmps_sampled import ComplexSampledMPSBornMachine
        return ComplexSampledMPSBornMachine
    if name == "PurifiedSampledMPSBornMachine":
        from .born_machine_lps_sampled import PurifiedSampledMPSBornMachine
        return PurifiedSampledMPSBornMachine
    if name == "TreeSampledBornMachine":
        from .born_machine_ttn_sampled import TreeSampledBornMachine
        return TreeSampledBornMachine
    if name == "SampledELBOVariationalInference":
        from .elbo_vi_sampled import SampledELBOVariationalInference
        return SampledELBOVariationalInference
    if name == "SampledKSDVariationalInference":
        from .ksd_vi_sampled import SampledKSDVariationalInference
        return SampledKSDVariationalInference
    if name == "SampledFisherPreconditioner":
        from .natural_gradient import SampledFisherPreconditioner
        return SampledFisherPreconditioner
    if name == "SampleSpaceFisherPreconditioner":
        from .natural_gradient import SampleSpaceFisherPreconditioner
        return SampleSpaceFisherPreconditioner
    if name == "CGFisherPreconditioner":
        from .natural_gradient import CGFisherPreconditioner
        return CGFisherPreconditioner
    if name == "AmortisedMPSInference":
        from .amortised_vi_sampled import AmortisedMPSInference
        return AmortisedMPSInference
    if name == "HammingMixtureKernel":
        from .hamming_kernel import HammingMixtureKernel
        return HammingMixtureKernel
    if name == "MMDObjective":
        from .mmd_objective import MMDObjective
        return MMDObjective
    if name == "QuantumMMDTrainer":
        from .mmd_quantum import QuantumMMDTrainer
        return QuantumMMDTrainer
    if name == "ClassicalMMDTrainer":
        from .mmd_classical import ClassicalMMDTrainer
        return ClassicalMMDTrainer
    if name == "SampledMMDTrainer":
        from .mmd_sampled import SampledMMDTrainer
        return SampledMMDTrainer
    raise AttributeError(name)
