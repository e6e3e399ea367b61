"""Every entry point beside work in flight: the table of (holder, other) pairs and what runs them.

A HOLDER is work the caller has begun on the context and not yet collected -- proofs in flight, commits in flight, a split-phase
session.  An OTHER is any other operation of the Python mirror on the same context.  include/zkhip.h ("Calls beside work in flight")
states the rule: the other call either REFUSES (ZKHIP_ERR_BUSY, nothing launched, reserved, freed or written) or SERVES (the bits it
delivers on an idle context), and the holder's results are what they would have been either way.

This module is the table (no GPU and no oracle at import: tests/test_inflight_cases_cpu.py reads it on a machine without a device)
and, below it, the code that runs a cell (everything that needs the device is imported inside the functions;
tests/test_gpu_beside_in_flight.py calls it; tools/stress_parity.py has a randomised case of the same rule).
"""
import hashlib
import time

SERVES, BUSY = "serves", "busy"

# ---- holders ------------------------------------------------------------------------------------------------------------------
# name -> (what is in flight, the mirror methods that begin and collect it)
HOLDERS = {
    "H1": ("one Sumcheck.prove_begin() of 2^12 entries", ("Sumcheck.poly_sum", "Sumcheck.prove_begin", "PendingProof.wait")),
    "H2": ("eight proofs in flight, 2^3, 2^9, 2^12 and 2^16 entries twice over: every result slot is taken",
           ("Sumcheck.poly_sum", "Sumcheck.prove_begin", "PendingProof.wait")),
    "H3": ("four proofs of 2^19 entries under ZKHIP_OVERLAP_MIN_LOG=19 (a process of its own): from the third on the big fold waits in "
           "zkhip_ctx::deferred", ("Sumcheck.poly_sum", "Sumcheck.prove_begin", "PendingProof.wait")),
    "H4": ("one MultilinearKZG.commitment_begin on a plain 2^10 SRS: async slot 0, its terms in msm_pin[0]",
           ("MultilinearKZG.commitment_begin", "_commit_begin", "PendingCommitment.wait")),
    "H5": ("three commits in flight against a precomputed table", ("MultilinearKZG.commitment_begin", "_commit_begin", "PendingCommitment.wait")),
    "H6": ("a live distributed.HipSumcheckEngine on a 2^12 table", ("HipSumcheckEngine.__init__", "ShardedSumcheck.prove")),
    "H7": ("a live distributed.HipComposedEngine (multi, term sizes [2, 2], 2^10 entries), begun and not yet driven: tables of this size fit the "
           "session's replicated tail, so it has no round of its own before it is collected",
           ("HipComposedEngine.__init__", "ShardedComposedSumcheck.prove")),
}
PROOF_HOLDERS = ("H1", "H2", "H3")            # proofs in flight: they hold the result slots, not the workspace
WORKSPACE_HOLDERS = ("H4", "H5", "H6", "H7")  # commits in flight and sessions: the workspace is lent
CHILD_HOLDERS = {"H3": {"ZKHIP_OVERLAP_MIN_LOG": "19"}}   # holders that need a process of their own, and its environment

# ---- others -------------------------------------------------------------------------------------------------------------------
# name -> (the mirror methods the cell goes through, qualified as the package defines them).  tests/test_inflight_cases_cpu.py reads
# the zkhip_* calls of these methods off the package's source: every declaration of include/zkhip.h must be reached by some row.
OTHERS = {
    # Multilinear
    "ml.partial_evaluation": ("Multilinear.partial_evaluation",),
    "ml.partial_evaluations": ("Multilinear.partial_evaluations",),
    "ml.evaluation_2_12": ("Multilinear.evaluation",),
    "ml.evaluation_2_17": ("Multilinear.evaluation",),                # the one-pass form
    "ml.half_sums": ("Multilinear._half_sums",),
    "ml.distinct": ("Multilinear.add_distinct", "Multilinear.mul_distinct"),
    "ml.elementwise": ("Multilinear._elementwise",),
    "ml.to_bytes": ("Multilinear.to_bytes",),
    "ml.add_to_back": ("Multilinear.add_to_back", "Multilinear.add_to_front"),
    # Sumcheck
    "sc.poly_sum_prove": ("Sumcheck.poly_sum", "Sumcheck.prove"),
    "sc.prove_batch": ("Sumcheck.prove_batch",),
    "csc.prove": ("ComposedSumcheck.calculate_poly_sum", "ComposedSumcheck.prove"),
    "csc.prove_batch": ("ComposedSumcheck.prove_batch",),
    "cm.element_wise": ("ComposedMultilinear._element_wise",),
    "mcs.prove": ("MultiComposedSumcheckProver._prove",),
    "mcs.prove_partial": ("MultiComposedSumcheckProver.calculate_poly_sum", "MultiComposedSumcheckProver._prove"),
    # Circuit and GKR
    "circuit.evaluation": ("Circuit.evaluation",),
    "circuit.add_mult_mle": ("Circuit.add_mult_mle",),
    "gkr.prove_d4": ("GKRProtocol.prove", "_DeviceCircuit.__init__"),
    "gkr.prove_d8": ("GKRProtocol.prove",),                           # its proof block outgrows a small commit's pinned terms
    "gkr.prove_batch": ("GKRProtocol.prove_batch",),
    "gkr.prove_sharded": ("GKRProtocol.prove_sharded",),
    # setup and KZG
    "srs.setup": ("TrustedSetup.setup",),
    "srs.precompute": ("TrustedSetup.precompute", "TrustedSetup._drop_tables"),
    "srs.precompute_open": ("TrustedSetup.folded", "TrustedSetup.precompute_open"),
    "kzg.commitment": ("MultilinearKZG.commitment", "_commit", "TrustedSetup._fingerprint"),
    "kzg.commitment_batch": ("commit_batch",),
    "kzg.open_cached": ("MultilinearKZG.open",),
    "kzg.open_uncached": ("MultilinearKZG.open",),
    "kzg.open_batch": ("MultilinearKZG.open_batch",),
    "kzg.verify": ("MultilinearKZG.verify_batch", "TrustedSetup.prepared_lines"),
    "kzg.pairing": ("pairing", "g2_prepare"),
    "ukzg.generate_srs": ("UnivariateKZG.generate_srs",),
    "ukzg.commitment": ("UnivariateKZG.commitment", "_commit"),
    "ukzg.open": ("UnivariateKZG.open",),
    "ukzg.verify_batch": ("UnivariateKZG.verify_batch", "TrustedSetup.prepared_lines"),
    # transforms and transcript
    "domain.fft_2_8": ("Domain._transform",),
    "domain.fft_2_12": ("Domain._transform",),
    "domain.fft_batch": ("Domain._transform_batch",),
    "ueval.multiply": ("UnivariateEval.multiply",),
    "ueval.multiply_batch": ("UnivariateEval.multiply_batch",),
    "dense.evaluate": ("DenseUnivariatePolynomial.evaluate",),
    "dense.degree": ("DenseUnivariatePolynomial.degree",),
    "transcript.challenge": ("DeviceFiatShamirTranscript.challenge",),
    # PLONK
    "plonk.vpi": ("_Key.__init__", "_Key.close"),
    "plonk.prove": ("PlonkProver.prove",),
    "plonk.prove_batch": ("PlonkProver.prove_batch",),
    "plonk.verify": ("PlonkVerifier.verify",),
    "plonk.verify_batch": ("PlonkVerifier.verify_batch",),
    # context
    "ctx.synchronize": ("Context.synchronize",),
}
OTHER_NAMES = tuple(OTHERS)

# ---- which call decides a cell, and the header line that says so ---------------------------------------------------------------
# Citations are phrases of include/zkhip.h (the CPU test looks them up, whitespace-insensitively).
CITE_SLOTS = "While a proof is in flight zkhip_sumcheck_prove returns ZKHIP_ERR_BUSY"
CITE_BATCH_SLOTS = "proofs are in flight or a split-phase session holds the workspace"
CITE_COMMIT = "commit is in flight the context's workspace is lent (other entry points that need it return ZKHIP_ERR_BUSY)"
CITE_SESSION = "every other entry point that needs that workspace returns ZKHIP_ERR_BUSY"
CITE_USERS = "WORKSPACE USERS:"          # the list of entry points that need the workspace
CITE_FREE = "NO WORKSPACE:"              # the list of entry points that are served beside every holder
CITE_PROOFS_SERVE = "Proofs in flight hold the result slots of the basic prover and nothing else"

# Others that end in an entry point of the header's WORKSPACE USERS list: refused beside H4 .. H7.  (The CPU test derives the same set
# from the header's list and the package's source, and fails when the two disagree.)
NEEDS_WORKSPACE = frozenset(OTHER_NAMES) - frozenset((
    "ml.partial_evaluation", "ml.half_sums", "ml.distinct", "ml.elementwise", "ml.to_bytes", "ml.add_to_back", "cm.element_wise",
    "gkr.prove_batch", "dense.evaluate", "dense.degree", "ctx.synchronize"))
NEEDS_RESULT_SLOTS = {"sc.poly_sum_prove": CITE_SLOTS, "sc.prove_batch": CITE_BATCH_SLOTS}


def expected(holder, other):
    """(outcome, the header phrase it was read from) of `other` while `holder` is live"""
    if holder not in HOLDERS or other not in OTHERS:
        raise KeyError((holder, other))
    if holder in PROOF_HOLDERS:
        if other in NEEDS_RESULT_SLOTS:
            return BUSY, NEEDS_RESULT_SLOTS[other]
        return SERVES, CITE_PROOFS_SERVE
    if other in NEEDS_WORKSPACE:
        return BUSY, CITE_USERS
    return SERVES, CITE_FREE


TABLE = {(h, o): expected(h, o) for h in HOLDERS for o in OTHERS}

# Entry points whose header promises untouched outputs on refusal: the raw-ABI cells under H4 and H6 (test_gpu_beside_in_flight.py)
PROMISE_UNTOUCHED = ("zkhip_sumcheck_prove_batch", "zkhip_composed_prove_batch", "zkhip_domain_transform_batch",
                     "zkhip_univariate_multiply_batch", "zkhip_plonk_prove_batch", "zkhip_plonk_verify_batch", "zkhip_kzg_open_batch")

# ... and those that say so since the refusal was moved in front of everything else they do (profiles/inflight/NOTES.md)
PROMISED_SINCE = ("zkhip_univariate_kzg_open", "zkhip_gkr_prove_circuit", "zkhip_kzg_open_tables", "zkhip_kzg_verify_batch", "zkhip_plonk_prove",
                  "zkhip_plonk_verify", "zkhip_circuit_add_mult_mle")

# ... and entry points of the header's lists that no cell calls beside a lent workspace (no mirror method binds them, or the mirror's
# method is refused at an earlier call of its own): called by the raw ABI beside H4 and H6, inputs built beforehand
RAW_REFUSED = ("zkhip_gkr_prove", "zkhip_srs_level_tables", "zkhip_srs_multilinear_g2", "zkhip_srs_univariate_g2", "zkhip_pairing",
               "zkhip_pairing_prepared", "zkhip_univariate_kzg_verify_batch", "zkhip_ntt", "zkhip_kzg_open", "zkhip_mc_begin")
RAW_SERVED = ("zkhip_plonk_vkey_create", "zkhip_gkr_layer_tables", "zkhip_circuit_create")

# Declarations of include/zkhip.h that take a context, key, circuit or comm and have no row, each with its reason
EXCLUDED = {
    "zkhip_ctx_create": "makes the context: there is no holder before it",
    "zkhip_ctx_destroy": "ends the context: it drains every holder (tests/test_gpu_threads.py destroys contexts with work in flight)",
    "zkhip_ctx_set_stream": "the mirror calls it when torch's current stream changes; the cells keep one stream",
    "zkhip_malloc": "allocator for hosts without one: no context state", "zkhip_free": "allocator for hosts without one",
    "zkhip_memcpy_h2d": "allocator-side copy helper: no context state", "zkhip_memcpy_d2h": "allocator-side copy helper",
    "zkhip_profile_enable": "diagnostics", "zkhip_profile_read": "diagnostics", "zkhip_profile_timeline": "diagnostics",
    "zkhip_debug_read_stamps": "diagnostics",
    "zkhip_gkr_prove": "the one-shot form, which the mirror does not bind: called by the raw ABI (RAW_REFUSED)",
    "zkhip_circuit_destroy": "releases a circuit's own arrays",
    "zkhip_gkr_layer_tables": "the stepwise prover's table builder, no cell goes through it: called by the raw ABI (RAW_SERVED)",
    "zkhip_gkr_layer_tables_sharded": "sharded transports: a rank's table builder",
    "zkhip_mle_block_sums_total": "reads the total poly_sum() deferred, for tables from 2^19 entries: part of holder H3's poly_sum, not a call beside it",
    "zkhip_mc_begin": "the mirror begins its sessions through zkhip_mc_begin_ex (H7): called by the raw ABI (RAW_REFUSED)",
    "zkhip_comm_create": "sharded transports", "zkhip_comm_create_rccl": "sharded transports", "zkhip_comm_destroy": "sharded transports",
    "zkhip_comm_all_gather": "sharded transports", "zkhip_comm_stats": "sharded transports", "zkhip_comm_inject_failure": "sharded transports",
    "zkhip_comm_measure": "sharded transports", "zkhip_sumcheck_prove_sharded": "sharded transports",
    "zkhip_composed_prove_sharded": "sharded transports", "zkhip_multi_composed_prove_sharded": "sharded transports",
    "zkhip_kzg_commit_sharded": "sharded transports",
    "zkhip_kzg_open": "the mirror calls zkhip_kzg_open_tables: called by the raw ABI (RAW_REFUSED)",
    "zkhip_ntt": "the mirror's Domain goes through zkhip_domain_transform: called by the raw ABI (RAW_REFUSED)",
    "zkhip_pointwise_mul": "not bound by the mirror",
    "zkhip_plonk_vkey_destroy": "releases a key's own buffers",
    "zkhip_plonk_vkey_create": "the mirror keeps one verifier key per (context, circuit), built before the holders begin: called by the raw ABI (RAW_SERVED)",
    "zkhip_plonk_batch_chunk": "diagnostics: reads the key",
}


# ================================================================================================================================
# running a cell (GPU): everything below imports the device side lazily
# ================================================================================================================================
def canon(x):
    """a digest of a result: arrays by dtype, shape and bytes, the mirror's result objects field by field"""
    import numpy as np
    h = hashlib.sha256()

    def feed(v):
        if v is None or isinstance(v, (bool, int, str)):
            h.update(repr(v).encode())
        elif isinstance(v, (bytes, bytearray)):
            h.update(b"b%d:" % len(v))
            h.update(bytes(v))
        elif isinstance(v, np.generic):
            h.update(repr(v.item()).encode())
        elif isinstance(v, np.ndarray):
            a = np.ascontiguousarray(v)
            h.update(("a%s%s:" % (a.dtype.str, a.shape)).encode())
            h.update(a.tobytes())
        elif hasattr(v, "data_ptr") and hasattr(v, "cpu"):
            feed(v.cpu().numpy())
        elif isinstance(v, (list, tuple)):
            h.update(b"l%d:" % len(v))
            for i in v:
                feed(i)
        else:
            name = type(v).__name__
            h.update(name.encode())
            if name == "MultiComposedSumcheckProof":
                feed(v.to_bytes())
                feed(v.sum)
            elif name == "PlonkProof":
                from zk_cryptography_amd import plonk
                for f in plonk.PROOF_POINTS + plonk.PROOF_SCALARS:
                    feed(getattr(v, f))
            else:
                for f in _FIELDS[name]:
                    feed(getattr(v, f))
    feed(x)
    return h.hexdigest()


_FIELDS = {
    "G1Affine": ("xy", "infinity"), "Multilinear": ("evaluations",), "SumcheckProof": ("sum", "univariate_poly"),
    "ComposedSumcheckProof": ("round_polys",), "GKRProof": ("sumcheck_proofs", "wb_s", "wc_s", "w_0_mle", "_challenges"),
    "MultilinearKZGProof": ("evaluation", "proofs"), "UnivariateKZGProof": ("evaluation", "proof"),
    "DenseUnivariatePolynomial": ("coefficients",),
}


class Env:
    """inputs, mirror objects and oracle results shared by every cell (built once per process)"""


def _affine_eq(ora, point, jac):
    import numpy as np
    want = ora.g1_to_affine(jac)
    return bool(point.infinity) == bool(want[12]) and (point.infinity or np.array_equal(point.xy, want[:12]))


def make_env(zk, ora, holders=tuple(HOLDERS)):
    """Everything the cells share.  The oracle's results for the holders are computed here, once."""
    import random

    import numpy as np
    import torch
    from zk_cryptography_amd import _native as N, distributed as D, kzg as K
    import gkr_cases as G
    import plonk_model as PL
    import pairing_model as PM
    from test_gpu_plonk import blinding, package_inputs, srs_for
    from test_gpu_pairing import g1 as pm_g1, g2 as pm_g2

    e = Env()
    e.zk, e.ora, e.N, e.D, e.K, e.np, e.torch, e.G, e.PL, e.PM = zk, ora, N, D, K, np, torch, G, PL, PM
    e.package_inputs = package_inputs
    rf = ora.random_fr
    e.ctx = N.Context.get()
    e.comm = D.Comm.get(e.ctx, 1, 0)
    ML = zk.Multilinear
    # Multilinear
    e.t12, e.t17 = rf(1 << 12, 61001), rf(1 << 17, 61002)
    e.p12, e.p17 = ML(e.t12), ML(e.t17)
    e.pts12, e.pts17 = rf(12, 61003), rf(17, 61004)
    e.ta, e.tb = rf(16, 61005), rf(8, 61006)
    e.pa, e.pb = ML(e.ta), ML(e.tb)
    e.tc = rf(16, 61008)
    e.pc = ML(e.tc)
    # sumcheck provers
    e.t10 = rf(1 << 10, 61007)
    e.p10 = ML(e.t10)
    e.tb8 = [rf(1 << 8, 61010 + b) for b in range(4)]
    e.pb8 = [ML(t) for t in e.tb8]
    e.tc10 = [rf(1 << 10, 61020 + q) for q in range(2)]
    e.cm10 = zk.ComposedMultilinear([ML(t) for t in e.tc10])
    e.tcb = [[rf(1 << 8, 61030 + 2 * b + q) for q in range(2)] for b in range(3)]
    e.cmb = [zk.ComposedMultilinear([ML(t) for t in pair]) for pair in e.tcb]
    e.tm8 = [rf(1 << 8, 61040 + q) for q in range(4)]
    e.mc8 = [zk.ComposedMultilinear([ML(e.tm8[0]), ML(e.tm8[1])]), zk.ComposedMultilinear([ML(e.tm8[2]), ML(e.tm8[3])])]
    e.mc8_sum = ora.multi_composed_sum(np.stack(e.tm8), [2, 2])
    # circuits
    e.layers4, e.layers8 = G.random_circuit(4), G.random_circuit(8)
    e.cir4, e.cir8 = zk.Circuit.from_tuples(e.layers4), zk.Circuit.from_tuples(e.layers8)
    e.cir3 = zk.Circuit.from_tuples(G.CIRCUIT_3["layers"])
    e.in4 = [rf(16, 61050 + b) for b in range(3)]
    e.in8 = rf(256, 61060)
    e.ev4 = [e.cir4.evaluation(i) for i in e.in4]
    e.ev8 = e.cir8.evaluation(e.in8)
    e.want_ev4 = [ora.circuit_evaluation(e.layers4, i) for i in e.in4]
    e.want_ev8 = ora.circuit_evaluation(e.layers8, e.in8)
    # KZG, multilinear: an SRS of 2^6 points with its G2 half, one with caches and one without
    e.tau6 = rf(6, 61070)
    e.srs6 = zk.TrustedSetup.setup(e.tau6, g2=True)
    e.srs6_plain = zk.TrustedSetup(e.srs6.powers_of_tau_in_g1, e.srs6.inf)
    e.osrs6 = ora.kzg_multilinear_srs_g1(e.tau6)
    e.t6, e.t6b = rf(1 << 6, 61071), rf(1 << 6, 61072)
    e.p6, e.p6b = ML(e.t6), ML(e.t6b)
    e.pts6, e.pts6b = rf(6, 61073), rf(6, 61074)
    e.tau5 = rf(5, 61075)
    e.commit6 = zk.MultilinearKZG.commitment(e.p6, e.srs6)
    e.open6 = zk.MultilinearKZG.open(e.p6, e.pts6, e.srs6)
    bad = zk.MultilinearKZGProof(zk.Fr.from_int(7).reshape(4), e.open6.proofs)
    e.open6_bad = bad
    # KZG, univariate
    e.utau = rf(1, 61080)[0]
    e.usrs = zk.UnivariateKZG.generate_srs(e.utau, 63, g2=True)
    e.ousrs = ora.kzg_univariate_srs_g1(e.utau, 63)
    e.ucoef = rf(64, 61081)
    e.upoly = zk.DenseUnivariatePolynomial(e.ucoef)
    e.uz = rf(1, 61082)[0]
    e.ucommit = zk.UnivariateKZG.commitment(e.upoly, e.usrs)
    e.uopen = zk.UnivariateKZG.open(e.upoly, e.uz, e.usrs)
    e.uopen_bad = zk.UnivariateKZGProof(zk.Fr.from_int(9).reshape(4), e.uopen.proof)
    # pairing
    e.pm_p, e.pm_q = PM.M.g1_mul(PM.M.G1, 11), PM.g2_mul(PM.G2, 13)
    e.pair_p, e.pair_q = pm_g1(zk, e.pm_p), pm_g2(zk, e.pm_q)
    # transforms
    e.f200, e.f4096 = rf(200, 61090), rf(1 << 12, 61091)
    e.fb = np.stack([rf(100, 61092 + b) for b in range(3)])
    e.ma, e.mb = rf(33, 61095), rf(20, 61096)
    e.mba = [rf(33, 61100 + b) for b in range(3)]
    e.mbb = [rf(20, 61110 + b) for b in range(3)]
    dc = rf(1000, 61097).copy()
    dc[-3:] = 0
    e.dcoef = dc
    e.dpoly = zk.DenseUnivariatePolynomial(dc)
    e.dz = rf(1, 61098)[0]
    # PLONK: one structure of 8 rows, three witnesses
    n, seed = 8, 8
    e.pl_n, e.pl_tau = n, 17 + seed
    e.pl_wits = []
    for b in range(3):
        cpi, wit = PL.random_circuit(n, random.Random(seed), random.Random(900 + 7 * seed + b))
        e.pl_cpi = cpi
        e.pl_wits.append(wit)
    e.pl_c, _ = package_inputs(zk, e.pl_cpi, e.pl_wits[0])
    e.pl_srs = srs_for(zk, e.pl_tau, n)
    e.pl_bl = [blinding(1000 * seed + b) for b in range(3)]
    e.pl_wobj = [zk.Witness(w["a"], w["b"], w["c"], w["public_poly"]) for w in e.pl_wits]
    e.pl_prover = zk.PlonkProver(e.pl_c, e.pl_srs)
    e.pl_vpi = zk.VerifierPreprocessedInput.vpi(e.pl_srs, e.pl_c)
    e.pl_proofs = e.pl_prover.prove_batch(e.pl_wobj, blindings=e.pl_bl)
    from zk_cryptography_amd import plonk
    fields = {f: getattr(e.pl_proofs[0], f) for f in plonk.PROOF_POINTS + plonk.PROOF_SCALARS}
    fields["a_s_poly_zeta"] = (fields["a_s_poly_zeta"] + 1) % PL.R
    e.pl_bad = zk.PlonkProof(**fields)
    e.pl_pubs = [w["public_poly"] for w in e.pl_wits]

    # ---- the holders' inputs and what the oracle says they deliver
    e.h_proofs = {}

    def proof_case(log_n, seed_):
        t = rf(1 << log_n, seed_)
        e.h_proofs[seed_] = (ML(t), ora.sumcheck_prove(t))
        return seed_
    e.h1 = [proof_case(12, 62001)] if "H1" in holders else []
    e.h2 = [proof_case(l, 62010 + i) for i, l in enumerate((3, 9, 12, 16, 3, 9, 12, 16))] if "H2" in holders else []
    e.h3 = [proof_case(19, 62020 + i) for i in range(4)] if "H3" in holders else []
    e.h_tau = rf(10, 62030)
    e.h_srs_plain = zk.TrustedSetup.setup(e.h_tau)
    e.h_srs_table = zk.TrustedSetup(e.h_srs_plain.powers_of_tau_in_g1.clone(), e.h_srs_plain.inf.clone()).precompute()
    e.h_osrs = ora.kzg_multilinear_srs_g1(e.h_tau)
    e.h_ct = [rf(1 << 10, 62040 + i) for i in range(4)]
    e.h_cp = [ML(t) for t in e.h_ct]
    h_affine = ora.g1_batch_to_affine(e.h_osrs)
    e.h_cwant = [ora.msm_pippenger(t, h_affine) for t in e.h_ct]        # (the oracle's own bucket method: its naive sum takes 0.5 s per commitment)
    e.h6_t = rf(1 << 12, 62050)
    e.h6_dev = torch.from_numpy(e.h6_t.view(np.int64)).cuda()
    e.h6_want = ora.sumcheck_prove(e.h6_t)
    e.h7_t = [rf(1 << 10, 62060 + q) for q in range(4)]
    e.h7_dev = [torch.from_numpy(t.view(np.int64)).cuda() for t in e.h7_t]
    e.h7_sum = ora.multi_composed_sum(np.stack(e.h7_t), [2, 2])
    e.h7_want = ora.multi_composed_prove(np.stack(e.h7_t), [2, 2], e.h7_sum, True)
    # the fresh proof and commitment at the end of every holder's test
    e.fresh_t = rf(1 << 11, 62070)
    e.fresh_want = ora.sumcheck_prove(e.fresh_t)
    e.idle, e.oracle_openings = {}, {}
    return e


# ---- the others: run(env) -> the result; check(env, result) holds the idle result against the oracle or model ---------------------
def _host(t):
    import numpy as np
    return t.cpu().numpy().view(np.uint64)


def _eq(a, b):
    import numpy as np
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b)


def _vec(e, fn, a, b):
    """the oracle's scalar operation, entry by entry"""
    return e.np.stack([fn(x, y) for x, y in zip(a, b)])


def _same_basic(e, got, want):
    (proof, ch), (s, rp, och) = got, want
    return _eq(proof.sum, s) and _eq(proof.univariate_poly, rp) and _eq(ch, och)


RUN, CHECK = {}, {}


def _other(name):
    def reg(fn):
        RUN[name] = fn
        return fn
    return reg


def _check(name):
    def reg(fn):
        CHECK[name] = fn
        return fn
    return reg


@_other("ml.partial_evaluation")
def _(e):
    return e.p12.partial_evaluation(e.pts12[0], 3)


@_check("ml.partial_evaluation")
def _(e, r):
    assert _eq(_host(r.evaluations), e.ora.mle_partial_evaluation(e.t12, e.pts12[0], 3))


@_other("ml.partial_evaluations")
def _(e):
    return e.p12.partial_evaluations(e.pts12[:5], [0, 2, 1, 0, 3])


@_check("ml.partial_evaluations")
def _(e, r):
    assert _eq(_host(r.evaluations), e.ora.mle_partial_evaluations(e.t12, e.pts12[:5], [0, 2, 1, 0, 3]))


@_other("ml.evaluation_2_12")
def _(e):
    return e.p12.evaluation(e.pts12)


@_check("ml.evaluation_2_12")
def _(e, r):
    assert _eq(r, e.ora.mle_evaluation(e.t12, e.pts12))


@_other("ml.evaluation_2_17")
def _(e):
    return e.p17.evaluation(e.pts17)


@_check("ml.evaluation_2_17")
def _(e, r):
    assert _eq(r, e.ora.mle_evaluation(e.t17, e.pts17))


@_other("ml.half_sums")
def _(e):
    return e.p12.split_poly_into_two_and_sum_each_part(), e.p12.sum_over_the_boolean_hypercube()


@_check("ml.half_sums")
def _(e, r):
    assert _eq(_host(r[0].evaluations), e.ora.mle_half_sums(e.t12)) and _eq(r[1], e.ora.mle_sum(e.t12))


@_other("ml.distinct")
def _(e):
    return e.pa.add_distinct(e.pb), e.pa.mul_distinct(e.pb)


@_check("ml.distinct")
def _(e, r):
    assert _eq(_host(r[0].evaluations), e.ora.mle_add_distinct(e.ta, e.tb)) and _eq(_host(r[1].evaluations), e.ora.mle_mul_distinct(e.ta, e.tb))


@_other("ml.elementwise")
def _(e):
    return e.pa + e.pc, e.pa - e.pc, e.pa * e.pts12[1]


@_check("ml.elementwise")
def _(e, r):
    o = e.ora
    assert _eq(_host(r[0].evaluations), _vec(e, o.fr_add, e.ta, e.tc)) and _eq(_host(r[1].evaluations), _vec(e, o.fr_sub, e.ta, e.tc))
    assert _eq(_host(r[2].evaluations), _vec(e, o.fr_mul, e.ta, e.np.tile(e.pts12[1], (16, 1))))


@_other("ml.to_bytes")
def _(e):
    return e.p12.to_bytes()


@_check("ml.to_bytes")
def _(e, r):
    assert r == e.ora.mle_to_bytes(e.t12)


@_other("ml.add_to_back")
def _(e):
    return e.pa.add_to_back(3), e.pa.add_to_front(2)


@_check("ml.add_to_back")
def _(e, r):
    assert _eq(_host(r[0].evaluations), e.ora.mle_add_to_back(e.ta, 3)) and _eq(_host(r[1].evaluations), e.ora.mle_add_to_front(e.ta, 2))


@_other("sc.poly_sum_prove")
def _(e):
    sc = e.zk.Sumcheck(e.p10)
    sc.poly_sum()
    return sc.prove()


@_check("sc.poly_sum_prove")
def _(e, r):
    assert _same_basic(e, r, e.ora.sumcheck_prove(e.t10))


@_other("sc.prove_batch")
def _(e):
    return e.zk.Sumcheck.prove_batch(e.pb8)


@_check("sc.prove_batch")
def _(e, r):
    assert len(r) == 4 and all(_same_basic(e, r[b], e.ora.sumcheck_prove(e.tb8[b])) for b in range(4))


@_other("csc.prove")
def _(e):
    return e.zk.ComposedSumcheck.calculate_poly_sum(e.cm10), e.zk.ComposedSumcheck(e.cm10).prove()


@_check("csc.prove")
def _(e, r):
    rp, ch = e.ora.composed_prove(e.np.stack(e.tc10))
    assert _eq(r[0], e.ora.composed_sum(e.np.stack(e.tc10))) and _eq(r[1][0].round_polys, rp) and _eq(r[1][1], ch)


@_other("csc.prove_batch")
def _(e):
    return e.zk.ComposedSumcheck.prove_batch(e.cmb)


@_check("csc.prove_batch")
def _(e, r):
    assert len(r) == 3
    for b in range(3):
        rp, ch = e.ora.composed_prove(e.np.stack(e.tcb[b]))
        assert _eq(r[b][0].round_polys, rp) and _eq(r[b][1], ch)


@_other("cm.element_wise")
def _(e):
    return e.cm10.element_wise_product(), e.cm10.element_wise_add()


@_check("cm.element_wise")
def _(e, r):
    got = [_host(x.evaluations if hasattr(x, "evaluations") else x) for x in r]
    assert _eq(got[0], _vec(e, e.ora.fr_mul, e.tc10[0], e.tc10[1])) and _eq(got[1], _vec(e, e.ora.fr_add, e.tc10[0], e.tc10[1]))


def _multi(e, partial):
    P = e.zk.MultiComposedSumcheckProver
    return (P.prove_partial if partial else P.prove)(e.mc8, e.mc8_sum)


def _multi_check(e, r, partial):
    rps, ch = e.ora.multi_composed_prove(e.np.stack(e.tm8), [2, 2], e.mc8_sum, partial)
    assert r[0].to_bytes() == e.ora.multi_composed_proof_bytes(rps) and _eq(r[1], ch) and _eq(r[0].sum, e.mc8_sum)


@_other("mcs.prove")
def _(e):
    return _multi(e, False)


@_check("mcs.prove")
def _(e, r):
    _multi_check(e, r, False)


@_other("mcs.prove_partial")
def _(e):
    return e.zk.MultiComposedSumcheckProver.calculate_poly_sum(e.mc8), _multi(e, True)


@_check("mcs.prove_partial")
def _(e, r):
    assert _eq(r[0], e.mc8_sum)
    _multi_check(e, r[1], True)


@_other("circuit.evaluation")
def _(e):
    return e.cir4.evaluation(e.in4[0])


@_check("circuit.evaluation")
def _(e, r):
    assert len(r) == 5 and all(_eq(_host(a), b) for a, b in zip(r, e.want_ev4[0]))


@_other("circuit.add_mult_mle")
def _(e):
    return e.cir3.add_mult_mle(1)


@_check("circuit.add_mult_mle")
def _(e, r):
    add, mul = e.ora.circuit_add_mult_mle(e.G.CIRCUIT_3["layers"], 1)
    assert _eq(_host(r[0].evaluations), add) and _eq(_host(r[1].evaluations), mul)


def _gkr_check(e, proof, layers, want_ev):
    assert e.G.gkr_proof_mismatches(e.ora, proof, e.ora.gkr_prove(layers, want_ev)) == []


@_other("gkr.prove_d4")
def _(e):
    return e.zk.GKRProtocol.prove(e.cir4, e.ev4[0])


@_check("gkr.prove_d4")
def _(e, r):
    _gkr_check(e, r, e.layers4, e.want_ev4[0])


@_other("gkr.prove_d8")
def _(e):
    return e.zk.GKRProtocol.prove(e.cir8, e.ev8)


@_check("gkr.prove_d8")
def _(e, r):
    assert e.G.gkr_proof_mismatches(e.ora, r, e.ora.gkr_prove_sparse(e.layers8, e.want_ev8)) == []      # (the dense oracle takes seconds at this depth)


@_other("gkr.prove_batch")
def _(e):
    return e.zk.GKRProtocol.prove_batch(e.cir4, e.ev4, max_lanes=2)


@_check("gkr.prove_batch")
def _(e, r):
    assert len(r) == 3
    for b in range(3):
        _gkr_check(e, r[b], e.layers4, e.want_ev4[b])


@_other("gkr.prove_sharded")
def _(e):
    return e.zk.GKRProtocol.prove_sharded(e.cir4, e.ev4[1], comm=e.comm)


@_check("gkr.prove_sharded")
def _(e, r):
    _gkr_check(e, r, e.layers4, e.want_ev4[1])


def _srs_g1_check(e, srs, want_jac):
    want = e.ora.g1_batch_to_affine(want_jac)
    assert _eq(_host(srs.powers_of_tau_in_g1), want[:, :12]) and _eq(srs.inf.cpu().numpy(), want[:, 12].astype(e.np.uint8))


@_other("srs.setup")
def _(e):
    s = e.zk.TrustedSetup.setup(e.tau5, g2=True)
    return s.powers_of_tau_in_g1, s.inf, s.powers_of_tau_in_g2, s.g2_inf


@_check("srs.setup")
def _(e, r):
    s = e.zk.TrustedSetup(*r)
    _srs_g1_check(e, s, e.ora.kzg_multilinear_srs_g1(e.tau5))
    got = s.g2_points()
    assert not any(q.infinity for q in got) and [q.coords() for q in got] == e.PM.multilinear_srs_g2(e.zk.Fr.to_ints(e.tau5))


@_other("srs.precompute")
def _(e):
    s = e.zk.TrustedSetup(e.srs6.powers_of_tau_in_g1, e.srs6.inf)
    table = s.precompute().table.clone()
    s.invalidate()
    return table


@_check("srs.precompute")
def _(e, r):
    # no model lays the table out: a commitment through this very table is the oracle's
    s = e.zk.TrustedSetup(e.srs6.powers_of_tau_in_g1, e.srs6.inf)
    s.precompute()
    assert _eq(_host(s.table), _host(r))
    got = e.K._commit(s.powers_of_tau_in_g1, s.inf, len(s), e.p6.evaluations, len(e.p6), True, s.table)
    assert _affine_eq(e.ora, got, e.ora.kzg_commitment(e.t6, e.osrs6, True))


@_other("srs.precompute_open")
def _(e):
    s = e.zk.TrustedSetup(e.srs6.powers_of_tau_in_g1, e.srs6.inf).precompute_open()
    return s.folded()[0], s.folded()[1], s.level_tables.clone()


@_check("srs.precompute_open")
def _(e, r):
    # level 0 of the folded SRS is S_0[j] = SRS[j] + SRS[32 + j]; the tables are held by the openings through them (kzg.open_cached)
    xy = _host(r[0])
    for j in (0, 17, 31):
        want = e.ora.g1_to_affine(e.ora.g1_add(e.osrs6[j], e.osrs6[32 + j]))
        assert _eq(xy[j], want[:12])
    assert _eq(_host(e.srs6.level_tables), _host(r[2]))


@_other("kzg.commitment")
def _(e):
    s = e.srs6
    return e.zk.MultilinearKZG.commitment(e.p6, s), e.K._commit(s.powers_of_tau_in_g1, s.inf, len(s), e.p6.evaluations, len(e.p6), True, None)


@_check("kzg.commitment")
def _(e, r):
    want = e.ora.kzg_commitment(e.t6, e.osrs6, True)
    assert _affine_eq(e.ora, r[0], want) and _affine_eq(e.ora, r[1], want)


_OFFSETS = [0, 1, 17, 64]


@_other("kzg.commitment_batch")
def _(e):
    return e.K.commit_batch(e.srs6.powers_of_tau_in_g1, e.srs6.inf, e.p6.evaluations, _OFFSETS)


@_check("kzg.commitment_batch")
def _(e, r):
    assert len(r) == 3
    for j in range(3):
        a, b = _OFFSETS[j], _OFFSETS[j + 1]
        assert _affine_eq(e.ora, r[j], e.ora.kzg_commitment(e.t6[a:b], e.osrs6[a:b], True))


def _open_check(e, proof, t, pts):
    key = (t.tobytes(), pts.tobytes())
    if key not in e.oracle_openings:
        e.oracle_openings[key] = e.ora.kzg_open(t, pts, e.osrs6)
    ev, proofs = e.oracle_openings[key]
    assert _eq(proof.evaluation, ev) and len(proof.proofs) == 6 and all(_affine_eq(e.ora, proof.proofs[i], proofs[i]) for i in range(6))


@_other("kzg.open_cached")
def _(e):
    return e.zk.MultilinearKZG.open(e.p6, e.pts6, e.srs6)


@_check("kzg.open_cached")
def _(e, r):
    _open_check(e, r, e.t6, e.pts6)


@_other("kzg.open_uncached")
def _(e):
    return e.zk.MultilinearKZG.open(e.p6b, e.pts6b, e.srs6_plain, cache_folded_srs=False)


@_check("kzg.open_uncached")
def _(e, r):
    _open_check(e, r, e.t6b, e.pts6b)


@_other("kzg.open_batch")
def _(e):
    return e.zk.MultilinearKZG.open_batch([e.p6, e.p6b, e.p6], [e.pts6, e.pts6b, e.pts6b], e.srs6)


@_check("kzg.open_batch")
def _(e, r):
    assert len(r) == 3
    _open_check(e, r[0], e.t6, e.pts6)
    _open_check(e, r[1], e.t6b, e.pts6b)
    _open_check(e, r[2], e.t6, e.pts6b)


@_other("kzg.verify")
def _(e):
    s = e.zk.TrustedSetup(e.srs6.powers_of_tau_in_g1, e.srs6.inf, e.srs6.powers_of_tau_in_g2, e.srs6.g2_inf)   # its lines are prepared in the call
    return [bool(v) for v in e.zk.MultilinearKZG.verify_batch([e.commit6, e.commit6], [e.pts6, e.pts6], [e.open6, e.open6_bad], s)]


@_check("kzg.verify")
def _(e, r):
    # the opening is the oracle's (kzg.open_cached), which the reference's verifier accepts; the other claims another evaluation
    # The model's verdicts with tau known, which needs no pairing (G1 and G2 have prime order): e(C - v G1, G2) == prod e(pi_i, (tau_i -
    # z_i) G2)  <=>  C - v G1 == sum (tau_i - z_i) pi_i.  (tests/pairing_model.py's multilinear_verify is seven pairings in python here;
    # tests/test_gpu_kzg_verify.py holds the device's verifier against it on three variables.)
    M, to_ints = e.PM.M, e.zk.Fr.to_ints
    tau, z = to_ints(e.tau6), to_ints(e.pts6)

    def model(proof):
        v = to_ints(e.np.asarray(proof.evaluation).reshape(1, 4))[0]
        lhs = M.g1_add(e.commit6.coords(), M.g1_mul(M.G1, (-v) % e.PM.R))
        rhs = None
        for pi, t, zi in zip(proof.proofs, tau, z):
            rhs = M.g1_add(rhs, M.g1_mul(None if pi.infinity else pi.coords(), (t - zi) % e.PM.R))
        return lhs == rhs
    assert r == [model(e.open6), model(e.open6_bad)] == [True, False]


@_other("kzg.pairing")
def _(e):
    prep = e.K.g2_prepare([e.pair_q])
    return e.zk.pairing([e.pair_p], [e.pair_q]), e.zk.pairing([e.pair_p], prepared=prep)


@_check("kzg.pairing")
def _(e, r):
    want = e.PM.f12_to_tower(e.PM.pairing(e.pm_p, e.pm_q))
    assert e.zk.gt_ints(r[0][0]) == want and e.zk.gt_ints(r[1][0]) == want


@_other("ukzg.generate_srs")
def _(e):
    s = e.zk.UnivariateKZG.generate_srs(e.utau, 15, g2=True)
    return s.powers_of_tau_in_g1, s.inf, s.powers_of_tau_in_g2, s.g2_inf


@_check("ukzg.generate_srs")
def _(e, r):
    _srs_g1_check(e, e.zk.TrustedSetup(r[0], r[1]), e.ora.kzg_univariate_srs_g1(e.utau, 15))
    assert _eq(_host(r[2]), _host(e.usrs.powers_of_tau_in_g2)[:16])      # the G2 powers: those of the longer SRS the verifier cell accepts with


@_other("ukzg.commitment")
def _(e):
    return e.zk.UnivariateKZG.commitment(e.upoly, e.usrs)


@_check("ukzg.commitment")
def _(e, r):
    assert _affine_eq(e.ora, r, e.ora.kzg_commitment(e.ucoef, e.ousrs, False))


@_other("ukzg.open")
def _(e):
    return e.zk.UnivariateKZG.open(e.upoly, e.uz, e.usrs)


@_check("ukzg.open")
def _(e, r):
    ev, proof = e.ora.univariate_kzg_open(e.ucoef, e.uz, e.ousrs)
    assert _eq(r.evaluation, ev) and _affine_eq(e.ora, r.proof, proof)


@_other("ukzg.verify_batch")
def _(e):
    s = e.zk.TrustedSetup(e.usrs.powers_of_tau_in_g1, e.usrs.inf, e.usrs.powers_of_tau_in_g2, e.usrs.g2_inf)
    return [bool(v) for v in e.zk.UnivariateKZG.verify_batch([e.ucommit, e.ucommit], [e.uz, e.uz], [e.uopen, e.uopen_bad], s)]


@_check("ukzg.verify_batch")
def _(e, r):
    assert r == [True, False]
    srs_g2 = e.PM.univariate_srs_g2(e.zk.Fr.to_ints(e.utau.reshape(1, 4))[0], 1)
    z, v = e.zk.Fr.to_ints(e.uz.reshape(1, 4))[0], e.zk.Fr.to_ints(e.uopen.evaluation.reshape(1, 4))[0]
    assert e.PM.univariate_verify(e.ucommit.coords(), z, v, e.uopen.proof.coords(), srs_g2)


@_other("domain.fft_2_8")
def _(e):
    return e.zk.Domain(256).fft(e.f200)


@_check("domain.fft_2_8")
def _(e, r):
    assert _eq(_host(r), e.ora.domain_fft(e.f200, 256))


@_other("domain.fft_2_12")
def _(e):
    return e.zk.Domain(1 << 12).fft(e.f4096)


@_check("domain.fft_2_12")
def _(e, r):
    assert _eq(_host(r), e.ora.domain_fft(e.f4096, 1 << 12))


@_other("domain.fft_batch")
def _(e):
    return e.zk.Domain(256).fft_batch(e.fb)


@_check("domain.fft_batch")
def _(e, r):
    got = _host(r)
    assert got.shape == (3, 256, 4) and all(_eq(got[b], e.ora.domain_fft(e.fb[b], 256)) for b in range(3))


@_other("ueval.multiply")
def _(e):
    D = e.zk.DenseUnivariatePolynomial
    return e.zk.UnivariateEval.multiply(D(e.ma), D(e.mb))


@_check("ueval.multiply")
def _(e, r):
    assert _eq(_host(r.coefficients), e.ora.univariate_multiply(e.ma, e.mb))


@_other("ueval.multiply_batch")
def _(e):
    D = e.zk.DenseUnivariatePolynomial
    return e.zk.UnivariateEval.multiply_batch([D(a) for a in e.mba], [D(b) for b in e.mbb])


@_check("ueval.multiply_batch")
def _(e, r):
    assert len(r) == 3 and all(_eq(_host(r[b].coefficients), e.ora.univariate_multiply(e.mba[b], e.mbb[b])) for b in range(3))


@_other("dense.evaluate")
def _(e):
    return e.dpoly.evaluate(e.dz)


@_check("dense.evaluate")
def _(e, r):
    assert _eq(r, e.ora.dense_evaluate(e.dcoef, e.dz))


@_other("dense.degree")
def _(e):
    return e.dpoly.degree()


@_check("dense.degree")
def _(e, r):
    assert r == 996


_MESSAGE = bytes(range(256)) * 2 + b"beside"


@_other("transcript.challenge")
def _(e):
    t = e.zk.DeviceFiatShamirTranscript()
    t.commit(_MESSAGE)
    first = t.challenge()
    t.commit(b"in flight")
    return first, t.challenge()


@_check("transcript.challenge")
def _(e, r):
    first = hashlib.sha256(_MESSAGE).digest()
    assert r[0] == first and r[1] == hashlib.sha256(first + b"in flight").digest()


@_other("plonk.vpi")
def _(e):
    c, _w = e.package_inputs(e.zk, e.pl_cpi, e.pl_wits[0])        # a preprocessed input of its own: its key is made in the call
    from zk_cryptography_amd import plonk
    key = plonk._Key(c, e.pl_srs)
    out = list(key.commitments)
    key.close()
    return out


@_check("plonk.vpi")
def _(e, r):
    assert r == e.pl_vpi._commitments()        # the key the verifier cells accept the model's proofs with


@_other("plonk.prove")
def _(e):
    return e.pl_prover.prove(e.pl_wobj[0], e.pl_bl[0])


def _plonk_model(e, b):
    if not hasattr(e, "_pl_model"):
        e._pl_model = {}
    if b not in e._pl_model:
        e._pl_model[b] = e.PL.prove(e.pl_cpi, e.pl_wits[b], e.pl_tau, e.pl_bl[b], n_srs=4 * e.pl_n + 1)
    return e._pl_model[b]


def _plonk_model_verdict(e, proof, b):
    """tests/plonk_model.py's verifier on a proof of witness b (its pairing-free form: the model knows tau)"""
    from test_gpu_plonk import proof_dict
    if not hasattr(e, "_pl_model_v"):
        e._pl_model_v = e.PL.vpi(e.pl_cpi, e.pl_tau)
    return e.PL.verify_tau(e.pl_n, proof_dict(proof), e._pl_model_v, e.pl_pubs[b], e.pl_tau)


@_check("plonk.prove")
def _(e, r):
    from test_gpu_plonk import proof_dict
    assert proof_dict(r) == _plonk_model(e, 0)


@_other("plonk.prove_batch")
def _(e):
    return e.pl_prover.prove_batch(e.pl_wobj, blindings=e.pl_bl)


@_check("plonk.prove_batch")
def _(e, r):
    from test_gpu_plonk import proof_dict
    assert len(r) == 3 and all(proof_dict(r[b]) == _plonk_model(e, b) for b in range(3))


@_other("plonk.verify")
def _(e):
    V = e.zk.PlonkVerifier
    return [V(e.pl_n, p, e.pl_srs, e.pl_vpi).verify(e.pl_pubs[0]) for p in (e.pl_proofs[0], e.pl_bad)]


@_check("plonk.verify")
def _(e, r):
    assert r == [_plonk_model_verdict(e, e.pl_proofs[0], 0), _plonk_model_verdict(e, e.pl_bad, 0)] == [True, False]


@_other("plonk.verify_batch")
def _(e):
    return e.zk.PlonkVerifier.verify_batch(e.pl_n, e.pl_proofs + [e.pl_bad], e.pl_srs, e.pl_vpi, e.pl_pubs + [e.pl_pubs[0]])


@_check("plonk.verify_batch")
def _(e, r):
    assert r == [_plonk_model_verdict(e, p, b) for p, b in zip(e.pl_proofs + [e.pl_bad], (0, 1, 2, 0))] == [True, True, True, False]


@_other("ctx.synchronize")
def _(e):
    return e.ctx.synchronize()


@_check("ctx.synchronize")
def _(e, r):
    assert r is None


def compute_idle(env, check=True):
    """the idle result of every other call, once: its digest, and (check) held against the oracle or model"""
    for name in OTHER_NAMES:
        r = RUN[name](env)
        if check:
            CHECK[name](env, r)
        env.idle[name] = canon(r)
        again = canon(RUN[name](env))
        assert again == env.idle[name], "%s is not a function of its inputs on an idle context" % name
    return env.idle


# ---- the holders: begin(env) -> state, collect(env, state) -> list of what differs from the oracle -------------------------------
def _begin_proofs(e, seeds):
    pend = []
    for s in seeds:
        sc = e.zk.Sumcheck(e.h_proofs[s][0])
        sc.poly_sum()
        pend.append((s, sc.prove_begin()))
    return pend


def _collect_proofs(e, pend):
    bad = []
    for s, p in pend:
        if not _same_basic(e, p.wait(), e.h_proofs[s][1]):
            bad.append("proof %d" % s)
    return bad


def _begin_commits(e, srs, count):
    return [e.zk.MultilinearKZG.commitment_begin(e.h_cp[i], srs) for i in range(count)]


def _collect_commits(e, pend):
    return ["commitment %d" % i for i, p in enumerate(pend) if not _affine_eq(e.ora, p.wait(), e.h_cwant[i])]


def _begin_h6(e):
    return e.D.HipSumcheckEngine(e.h6_dev)


def _collect_h6(e, eng):
    s, rp, ch = e.D.ShardedSumcheck(eng, 1, comm=e.comm).prove()
    ws, wrp, wch = e.h6_want
    return [] if (_eq(s, ws) and _eq(rp, wrp) and _eq(ch, wch)) else ["the session's proof"]


def _begin_h7(e):
    eng = e.D.HipComposedEngine([e.h7_dev[0:2], e.h7_dev[2:4]], 1, multi=True, claimed_sum=e.h7_sum)
    assert eng.local_len() <= eng.tail_capacity()      # no round to run ahead of the collection (HOLDERS["H7"]): the whole proof is its tail
    return eng


def _collect_h7(e, eng):
    rps, ch = e.D.ShardedComposedSumcheck(eng, 1, comm=e.comm).prove()
    want_rps, want_ch = e.h7_want
    from zk_cryptography_amd.composed import MultiComposedSumcheckProof, SparseUnivariatePolynomial
    proof = MultiComposedSumcheckProof([SparseUnivariatePolynomial(c, p) for c, p in rps], e.h7_sum)
    ok = proof.to_bytes() == e.ora.multi_composed_proof_bytes(want_rps) and _eq(ch, want_ch)
    return [] if ok else ["the session's proof"]


BEGIN = {
    "H1": lambda e: _begin_proofs(e, e.h1), "H2": lambda e: _begin_proofs(e, e.h2), "H3": lambda e: _begin_proofs(e, e.h3),
    "H4": lambda e: _begin_commits(e, e.h_srs_plain, 1), "H5": lambda e: _begin_commits(e, e.h_srs_table, 3),
    "H6": _begin_h6, "H7": _begin_h7,
}
COLLECT = {
    "H1": _collect_proofs, "H2": _collect_proofs, "H3": _collect_proofs, "H4": _collect_commits, "H5": _collect_commits,
    "H6": _collect_h6, "H7": _collect_h7,
}


class DeviceFault(RuntimeError):
    """a HIP runtime error came back from a cell: nothing more is to be started on the device"""


def run_cell(env, holder, other):
    """begin the holder, call the other, collect the holder, call the other again -> (outcome, what went wrong)"""
    N = env.N
    bad = []
    state = BEGIN[holder](env)
    outcome, got = None, None
    try:
        try:
            got = canon(RUN[other](env))
            outcome = SERVES
        except N.ZkhipError as ex:
            if ex.status == N.ERR_HIP:
                raise DeviceFault("%s beside %s: %s" % (other, holder, ex))
            outcome = BUSY if ex.status == N.ERR_BUSY else "status %s" % ex.status
            if outcome != BUSY:
                bad.append("%s beside %s: %s" % (other, holder, ex))      # (ZKHIP_ERR_TIMEOUT of a GKR call: reported with its cell)
    except DeviceFault:
        raise
    except BaseException:
        COLLECT[holder](env, state)         # a panic of the mirror (a shape, an index): the holder is ended, the error is the test's
        raise
    held = COLLECT[holder](env, state)
    bad += ["%s after %s (%s): %s differs from the oracle" % (holder, other, outcome, w) for w in held]
    if outcome == SERVES and got != env.idle[other]:
        bad.append("%s beside %s: served, but not the idle result" % (other, holder))
    if canon(RUN[other](env)) != env.idle[other]:
        bad.append("%s after %s ended: not the idle result" % (other, holder))
    return outcome, bad


def fresh_work_mismatches(env):
    """a fresh proof and a fresh commitment on the context, against the oracle"""
    bad = []
    sc = env.zk.Sumcheck(env.zk.Multilinear(env.fresh_t))
    sc.poly_sum()
    if not _same_basic(env, sc.prove(), env.fresh_want):
        bad.append("a fresh Sumcheck.prove")
    if not _affine_eq(env.ora, env.zk.MultilinearKZG.commitment(env.zk.Multilinear(env.h_ct[3]), env.h_srs_table), env.h_cwant[3]):
        bad.append("a fresh MultilinearKZG.commitment")
    return bad


def run_holder(env, holder, others=OTHER_NAMES):
    """every cell of one holder -> {"cells": {other: outcome}, "bad": [...], "seconds": wall time of the cells}"""
    cells, bad = {}, []
    t0 = time.perf_counter()
    for other in others:
        outcome, cell_bad = run_cell(env, holder, other)
        cells[other] = outcome
        bad += cell_bad
        want = TABLE[(holder, other)][0]
        if outcome != want and outcome in (SERVES, BUSY):
            bad.append("%s beside %s: %s, the table says %s" % (other, holder, outcome, want))
    bad += ["%s at the end: %s differs from the oracle" % (holder, w) for w in fresh_work_mismatches(env)]
    return {"holder": holder, "cells": cells, "bad": bad, "seconds": round(time.perf_counter() - t0, 3)}
