"""zk-cryptography_amd -- MI355X (gfx950) proving hot path of aagbotemi/zk-cryptography.

Host-side mirror (Python over ctypes) of the reference's Rust surfaces for the hot path:
    polynomial::Multilinear / MultilinearTrait      -> zk_cryptography_amd.polynomial
    sumcheck::{Sumcheck, ComposedSumcheck, MultiComposedSumcheckProver} -> .sumcheck
    kzg::{MultilinearKZG, UnivariateKZG}::{commitment, open, verify}, TrustedSetup (G1 and G2) -> .kzg
    circuit::Circuit, gkr::GKRProtocol::prove -> .gkr
    polynomial::univariate::{Domain, UnivariateEval} -> .univariate
    plonk::{compiler, protocol}, merlin::MerlinTranscript -> .plonk
    polynomial::DenseUnivariatePolynomial::{interpolate, evaluate}, shamir_secret_sharing -> .kzg, .shamir
Every operation runs hand-written HIP kernels in csrc/libzkhip.so through the C ABI of
include/zkhip.h; there is no CPU fallback (a missing library or GPU raises).
"""
from zk_cryptography_amd import _native  # noqa: F401
from zk_cryptography_amd.field import Fr  # noqa: F401
from zk_cryptography_amd.polynomial import Multilinear  # noqa: F401
from zk_cryptography_amd.sumcheck import Sumcheck, SumcheckProof  # noqa: F401
from zk_cryptography_amd.kzg import (DenseUnivariatePolynomial, G1Affine, G2Affine, MultilinearKZG, MultilinearKZGProof, TrustedSetup,  # noqa: F401
                                     UnivariateKZG, UnivariateKZGProof, gt_ints, pairing)
from zk_cryptography_amd.composed import (ComposedMultilinear, ComposedSumcheck, ComposedSumcheckProof,  # noqa: F401
                                          MultiComposedSumcheckProof, MultiComposedSumcheckProver,
                                          SparseUnivariatePolynomial)
from zk_cryptography_amd.univariate import Domain, UnivariateEval  # noqa: F401
from zk_cryptography_amd import shamir  # noqa: F401
from zk_cryptography_amd.gkr import (Circuit, CircuitLayer, DeviceFiatShamirTranscript, FiatShamirTranscript, Gate, GKRProof, GKRProtocol,  # noqa: F401
                                     SuccintGKRProof, SuccintGKRProtocol)
from zk_cryptography_amd.plonk import (AssemblyEqn, CommonPreprocessedInput, MerlinTranscript, PlonkProof, PlonkProver,  # noqa: F401
                                       PlonkRoundTranscript, PlonkVerifier, Program, VerifierPreprocessedInput, Witness)
