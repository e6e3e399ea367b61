"""GPU: PlonkProver::prove / PlonkVerifier::verify (zkhip_plonk_*) against the independent model of tests/plonk_model.py.
Every comparison is bit for bit.  With the blinding fixed the proof is a function of the inputs: all 15 fields and the six challenges
must equal the model's literal restatement (n = 4 -- the one size whose coset has D / n = 8 -- 8, 16, 64, 128); at n = 2^8, 2^10, 2^11,
2^12 and 2^16 the O(n) model checks every commitment that is an evaluation at the known tau, the t parts through
[t_low] + tau^n [t_mid] + tau^2n [t_high] = t(tau) G, the six evaluations and both opening commitments.  n = 1024 is the first full
workgroup of the grand product and the first coset of 2^12 points (the scaled transform replaces scale-and-pad), n = 2048 the first
chain of two workgroups.  The branches no size reaches are taken on purpose: a prebuilt shifted-SRS table above the small-SRS limit,
a key that keeps no coset cache (ZKHIP_PLONK_CACHE_BUDGET=0), and the verifier's checks of its arguments."""
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import plonk_model as PL  # noqa: E402

pytestmark = pytest.mark.gpu
M, R = PL.M, PL.R
P = M.P
PROGRAM_1 = (["e public"], {"e": 3})
PROGRAM_2 = (["x public", "c <== a * b", "f <== d * e", "g <== c + f", "x <== g * y"], {"x": 258, "a": 2, "b": 4, "d": 5, "e": 7, "y": 6})


@pytest.fixture(scope="module")
def zk():
    import zk_cryptography_amd as z
    return z


def blinding(seed):
    rng = random.Random(seed)
    return [rng.randrange(R) for _ in range(11)]


def to_affine(zk, pt):
    """a model point (x, y) / None -> G1Affine (Montgomery limbs)"""
    if pt is None:
        return zk.G1Affine(np.zeros(12, dtype=np.uint64), True)
    limbs = [(v * (1 << 384) % P >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for v in pt for k in range(6)]
    return zk.G1Affine(np.array(limbs, dtype=np.uint64), False)


def from_affine(pt):
    return None if pt.infinity else pt.coords()


def proof_dict(proof):
    return {f: (getattr(proof, f) if f.endswith("_zeta") else from_affine(getattr(proof, f))) for f in PL.PROOF_FIELDS}


def proof_object(zk, d):
    return zk.PlonkProof(**{f: (v if f.endswith("_zeta") else to_affine(zk, v)) for f, v in d.items()})


def package_inputs(zk, cpi, wit):
    c = zk.CommonPreprocessedInput(cpi["group_order"], cpi["q_l"], cpi["q_r"], cpi["q_m"], cpi["q_o"], cpi["q_c"],
                                   cpi["sigma_1"], cpi["sigma_2"], cpi["sigma_3"])
    return c, zk.Witness(wit["a"], wit["b"], wit["c"], wit["public_poly"])


def compiled(zk, constraints, assignment, n=8):
    program = zk.Program([zk.AssemblyEqn.eq_to_assembly(eq) for eq in constraints], n)
    wit = program.compute_witness_and_public_poly(dict(assignment))
    cpi = program.common_preprocessed_input()
    return ({f: getattr(cpi, f) for f in PL.CPI_FIELDS} | {"group_order": n},
            {"a": wit.a, "b": wit.b, "c": wit.c, "public_poly": wit.public_poly})


def case(zk, name):
    if name == "program_1":
        return compiled(zk, *PROGRAM_1)
    if name == "program_2":
        return compiled(zk, *PROGRAM_2)
    n = int(name.split("_")[1])
    return PL.random_circuit(n, random.Random(n), random.Random(1000 + n))     # a valid witness and sigma by construction


def srs_for(zk, tau, n):
    return zk.UnivariateKZG.generate_srs(zk.Fr.from_int(tau), 4 * n, g2=True)   # verifier.rs:205-206: group_order * 4


@pytest.mark.parametrize("name", ["program_1", "program_2", "random_4", "random_8", "random_16", "random_64", "random_128"])
def test_proof_equals_the_model_and_verdicts_agree(zk, name):
    cpi, wit = case(zk, name)
    n, tau, bl = cpi["group_order"], 6 + len(name), blinding(len(name))
    assert PL.gate_identity_holds(cpi, wit)
    want, want_ch = PL.prove(cpi, wit, tau, bl, n_srs=4 * n + 1, want_challenges=True)
    srs = srs_for(zk, tau, n)
    c, w = package_inputs(zk, cpi, wit)
    v = zk.VerifierPreprocessedInput.vpi(srs, c)
    model_v = PL.vpi(cpi, tau)
    assert [from_affine(p) for p in v._commitments()] == [model_v[f] for f in PL.CPI_FIELDS]
    assert v.x_2.coords() == model_v["x_2"]
    prover = zk.PlonkProver(c, srs, zk.PlonkRoundTranscript())
    proof = prover.prove(w, blinding=bl)
    got = proof_dict(proof)
    for f in PL.PROOF_FIELDS:
        assert got[f] == want[f], f
    assert tuple(prover.random_number[k] for k in ("beta", "gamma", "alpha", "zeta", "nu", "mu")) == want_ch
    from zk_cryptography_amd.plonk import compute_verifier_challenges
    assert compute_verifier_challenges(proof) == want_ch
    assert zk.PlonkVerifier(n, proof, srs, v).verify(w.public_poly) is True
    assert PL.verify_tau(n, want, model_v, wit["public_poly"], tau) is True
    for f in PL.PROOF_FIELDS:                                                   # every single-field tamper, and the model's verdict on it
        bad = PL.tamper(want, f)
        verdict = zk.PlonkVerifier(n, proof_object(zk, bad), srs, v).verify(w.public_poly)
        assert verdict is False and verdict == PL.verify_tau(n, bad, model_v, wit["public_poly"], tau), f
    wrong_public = [(wit["public_poly"][0] + 1) % R] + list(wit["public_poly"][1:])
    assert zk.PlonkVerifier(n, proof, srs, v).verify(wrong_public) is False


@pytest.mark.parametrize("name", ["program_2", "random_16"])
def test_default_blinding_randomises_and_verifies(zk, name):
    cpi, wit = case(zk, name)
    n = cpi["group_order"]
    srs = srs_for(zk, 9, n)
    c, w = package_inputs(zk, cpi, wit)
    v = zk.VerifierPreprocessedInput.vpi(srs, c)
    p1, p2 = zk.PlonkProver(c, srs).prove(w), zk.PlonkProver(c, srs).prove(w)
    assert proof_dict(p1) != proof_dict(p2)
    assert p1.as_commitment != p2.as_commitment and p1.t_high != p2.t_high
    for p in (p1, p2):
        assert zk.PlonkVerifier(n, p, srs, v).verify(w.public_poly) is True


@pytest.mark.parametrize("log_n", [8, 10, 11, 12, 16])
def test_large_circuits_against_the_linear_time_model(zk, log_n):
    n, tau, bl = 1 << log_n, 0xC0FFEE + log_n, blinding(log_n)
    cpi, wit = PL.random_circuit(n, random.Random(log_n), random.Random(77 + log_n))
    srs = zk.UnivariateKZG.generate_srs(zk.Fr.from_int(tau), n + 5, g2=True)    # n + 6 points: the least the prover accepts
    c, w = package_inputs(zk, cpi, wit)
    v = zk.VerifierPreprocessedInput.vpi(srs, c)
    proof = zk.PlonkProver(c, srs).prove(w, blinding=bl)
    assert PL.fast_check(cpi, wit, tau, bl, proof_dict(proof)) == []
    assert zk.PlonkVerifier(n, proof, srs, v).verify(w.public_poly) is True
    bad = proof_object(zk, PL.tamper(proof_dict(proof), "w_accumulator_poly_zeta"))
    assert zk.PlonkVerifier(n, bad, srs, v).verify(w.public_poly) is False


def test_errors(zk):
    from zk_cryptography_amd import _native as N
    cpi, wit = case(zk, "random_16")
    n = 16
    srs = srs_for(zk, 5, n)
    c, w = package_inputs(zk, cpi, wit)
    b_row = next(i for i in range(n) if (cpi["q_r"][i] + cpi["q_m"][i] * wit["a"][i]) % R)     # a row whose gate depends on b
    for column, row in (("a", 0), ("b", b_row), ("c", 5), ("public_poly", 1)):  # one witness cell changed -> ZKHIP_ERR_ARG
        cells = list(wit[column])
        cells[row] = (cells[row] + 1) % R
        _, w_bad = package_inputs(zk, cpi, dict(wit, **{column: cells}))
        with pytest.raises(N.ZkhipError) as e:
            zk.PlonkProver(c, srs).prove(w_bad, blinding=blinding(1))
        assert e.value.status == N.ERR_ARG
    sigma = list(cpi["sigma_1"])                                                # a permutation the witness does not respect
    sigma[0], sigma[1] = sigma[1], sigma[0]
    c_bad, _ = package_inputs(zk, dict(cpi, sigma_1=sigma), wit)
    with pytest.raises(N.ZkhipError) as e:
        zk.PlonkProver(c_bad, srs).prove(w, blinding=blinding(1))
    assert e.value.status == N.ERR_ARG
    zk.PlonkProver(c, srs).prove(w, blinding=blinding(1))                       # the untouched witness still proves
    short = zk.UnivariateKZG.generate_srs(zk.Fr.from_int(5), n + 4, g2=True)    # n + 5 points -> ZKHIP_ERR_INDEX
    c2, _ = package_inputs(zk, cpi, wit)
    with pytest.raises(IndexError):
        zk.PlonkProver(c2, short).prove(w, blinding=blinding(1))
    c3 = zk.CommonPreprocessedInput(12, *[[0] * 12 for _ in range(8)])          # not a power of two -> ZKHIP_ERR_SHAPE
    with pytest.raises(AssertionError):
        zk.PlonkProver(c3, srs).prove(zk.Witness(*[[0] * 12 for _ in range(4)]), blinding=blinding(1))


def test_key_reuse(zk):
    n = 64
    cpi, wit1 = PL.random_circuit(n, random.Random(5), random.Random(1))
    cpi2, wit2 = PL.random_circuit(n, random.Random(5), random.Random(2))
    assert cpi == cpi2 and wit1 != wit2
    srs = srs_for(zk, 21, n)
    shared, w1 = package_inputs(zk, cpi, wit1)
    _, w2 = package_inputs(zk, cpi, wit2)
    prover = zk.PlonkProver(shared, srs)
    got = [proof_dict(prover.prove(w, blinding=blinding(3 + i))) for i, w in enumerate((w1, w2))]
    assert len(shared._keys) == 1
    fresh = []
    for i, w in enumerate((w1, w2)):
        c, _ = package_inputs(zk, cpi, wit1)
        fresh.append(proof_dict(zk.PlonkProver(c, srs).prove(w, blinding=blinding(3 + i))))
    assert got == fresh and got[0] != got[1]
    assert got[0] == PL.prove(cpi, wit1, 21, blinding(3))


def test_prebuilt_table_above_the_small_srs_limit(zk):
    """commits through a shifted-SRS table built before the key, at a size the short path does not serve: the same proof, field for field"""
    n, tau, bl = 1 << 12, 0xBEEF, blinding(12)
    cpi, wit = PL.random_circuit(n, random.Random(12), random.Random(89))
    proofs = []
    for prebuilt in (True, False):
        srs = zk.UnivariateKZG.generate_srs(zk.Fr.from_int(tau), n + 5, g2=True)
        assert len(srs) > srs.SMALL_SRS
        if prebuilt:
            srs.precompute()
        c, w = package_inputs(zk, cpi, wit)
        v = zk.VerifierPreprocessedInput.vpi(srs, c)
        proof = zk.PlonkProver(c, srs).prove(w, blinding=bl)
        assert (srs.table is not None) == prebuilt
        assert zk.PlonkVerifier(n, proof, srs, v).verify(w.public_poly) is True
        proofs.append((proof_dict(proof), [from_affine(p) for p in v._commitments()]))
    for f in PL.PROOF_FIELDS:
        assert proofs[0][0][f] == proofs[1][0][f], f
    assert proofs[0][1] == proofs[1][1]


@pytest.mark.parametrize("n", [64, 4096])
def test_uncached_key(zk, n):
    """A key made under ZKHIP_PLONK_CACHE_BUDGET=0 holds no coset evaluations of its columns: every proof recomputes them into the work
    area, which the proof before it has used.  Its proofs equal a cached key's -- twice for one witness, then for another."""
    from zk_cryptography_amd.plonk import _key_for
    cpi, wit1 = PL.random_circuit(n, random.Random(n + 5), random.Random(1))
    _, wit2 = PL.random_circuit(n, random.Random(n + 5), random.Random(2))
    assert wit1 != wit2
    srs = zk.UnivariateKZG.generate_srs(zk.Fr.from_int(31), n + 5, g2=True)
    bl, bl2 = blinding(n), blinding(n + 1)
    uncached, w1 = package_inputs(zk, cpi, wit1)
    _, w2 = package_inputs(zk, cpi, wit2)
    before = os.environ.get("ZKHIP_PLONK_CACHE_BUDGET")
    os.environ["ZKHIP_PLONK_CACHE_BUDGET"] = "0"
    try:
        _key_for(uncached, srs)
    finally:
        if before is None:
            del os.environ["ZKHIP_PLONK_CACHE_BUDGET"]
        else:
            os.environ["ZKHIP_PLONK_CACHE_BUDGET"] = before
    prover = zk.PlonkProver(uncached, srs)
    first, second = proof_dict(prover.prove(w1, blinding=bl)), proof_dict(prover.prove(w1, blinding=bl))
    third = proof_dict(prover.prove(w2, blinding=bl2))
    assert len(uncached._keys) == 1                                             # all three from the key made above
    cached, _ = package_inputs(zk, cpi, wit1)
    want = proof_dict(zk.PlonkProver(cached, srs).prove(w1, blinding=bl))
    assert first == second and first == want
    fresh, _ = package_inputs(zk, cpi, wit1)
    assert third == proof_dict(zk.PlonkProver(fresh, srs).prove(w2, blinding=bl2)) and third != first
    v = zk.VerifierPreprocessedInput.vpi(srs, uncached)
    assert zk.PlonkVerifier(n, proof_object(zk, third), srs, v).verify(w2.public_poly) is True


def g1_mul_raw(pt, k):
    """k * pt without reducing k (M.g1_mul reduces mod r, which is the question here)"""
    acc = None
    while k:
        if k & 1:
            acc = M.g1_add(acc, pt)
        pt = M.g1_add(pt, pt)
        k >>= 1
    return acc


def point_outside_the_subgroup():
    """the first x = 1, 2, .. with x^3 + 4 a square: the cofactor is ~2^126, so such a curve point is not of order r"""
    x = 1
    while True:
        rhs = (x ** 3 + 4) % P
        y = pow(rhs, (P + 1) // 4, P)                                           # P = 3 mod 4
        if y * y % P == rhs:
            return x, y
        x += 1


def test_verifier_refuses_malformed_arguments(zk):
    """ZKHIP_ERR_ARG and no verdict for a point off the curve (in the proof, in the key), a curve point outside the order-r subgroup,
    and an evaluation that is not reduced; zkhip_plonk_challenges refuses the last as well"""
    import ctypes as C
    from zk_cryptography_amd import _native as N
    from zk_cryptography_amd import plonk
    n = 16
    cpi, wit = case(zk, "random_16")
    srs = srs_for(zk, 5, n)
    c, w = package_inputs(zk, cpi, wit)
    v = zk.VerifierPreprocessedInput.vpi(srs, c)
    proof = zk.PlonkProver(c, srs).prove(w, blinding=blinding(2))
    good = proof_dict(proof)
    pub = plonk._column(w.public_poly)
    ctx = N.Context.get(pub.device.index)
    vp = C.c_void_p

    def verify(proof_fields, vk_points, evals=None):
        xy, inf, ev = proof_object(zk, proof_fields)._arrays()
        if evals is not None:
            ev = evals
        vxy, vinf = plonk._points_arrays(vk_points)
        ok = C.c_uint8(0)
        st = N.lib().zkhip_plonk_verify(ctx.handle, C.c_size_t(n), vxy.ctypes.data_as(vp), vinf.ctypes.data_as(vp), xy.ctypes.data_as(vp),
                                        inf.ctypes.data_as(vp), ev.ctypes.data_as(vp), N.ptr(pub), N.ptr(srs.powers_of_tau_in_g2),
                                        N.ptr(srs.g2_inf), C.c_size_t(len(srs.powers_of_tau_in_g2)), C.byref(ok))
        assert st == N.ZKHIP_OK or ok.value == 0                                # an error never comes with "valid"
        N.check(st, "plonk verify")
        return bool(ok.value)

    vk = v._commitments()
    assert verify(good, vk) is True                                             # the route itself accepts the untouched proof
    x, y = good["t_mid"]
    off_curve = (x, (y + 1) % P)
    assert not M.on_curve(off_curve)
    stray = point_outside_the_subgroup()
    assert M.on_curve(stray) and g1_mul_raw(stray, R) is not None
    vx, vy = from_affine(vk[5])
    bad_vk = vk[:5] + [to_affine(zk, (vx, (vy + 1) % P))] + vk[6:]
    _, _, ev = proof._arrays()
    unreduced = ev.copy()
    unreduced[3] = [(R >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(4)]      # the limbs of r itself
    for fields, points, evals in ((dict(good, t_mid=off_curve), vk, None), (good, bad_vk, None),
                                  (dict(good, w_zeta_commitment=stray), vk, None), (good, vk, unreduced)):
        with pytest.raises(N.ZkhipError) as e:
            verify(fields, points, evals)
        assert e.value.status == N.ERR_ARG
    with pytest.raises(ValueError):                                             # the mirror class turns the status into ValueError
        zk.PlonkVerifier(n, proof_object(zk, dict(good, t_mid=off_curve)), srs, v).verify(w.public_poly)
    xy, inf, _ = proof._arrays()
    ch = np.zeros((6, 4), dtype=np.uint64)
    call = lambda e: N.lib().zkhip_plonk_challenges(xy.ctypes.data_as(vp), inf.ctypes.data_as(vp), e.ctypes.data_as(vp), ch.ctypes.data_as(vp))
    assert call(ev) == N.ZKHIP_OK
    with pytest.raises(N.ZkhipError) as e:
        N.check(call(unreduced), "plonk challenges")
    assert e.value.status == N.ERR_ARG
