"""The scalar algebra that zkhip_plonk_verify and zkhip_plonk_verify_batch share (csrc/plonk_scalars.hpp, host only) under
g++ -fsanitize=address,undefined, as a stand-alone program (tests/cpp/plonk_scalars_sanitize.cpp).  The program compares the function's
table for one fixed proof with literals from the python model; this test runs it and compares the table it prints with the model once
more, so a stale literal cannot pass either."""
import os
import random
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import plonk_model as PL  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M, R = PL.M, PL.R


def model_table(n, proof, pi_zeta):
    """the twenty scalars of the batch's G1 terms, restated from PL.verifier_points (order: csrc/plonk_verify_kernels.hpp)"""
    beta, gamma, alpha, zeta, nu, mu = PL.compute_verifier_challenges(proof)
    zn = pow(zeta, n, R)
    zh = (zn - 1) % R
    w = M.root_of_unity(n)
    l1 = PL.to_coefficient_poly(PL.l1_values(n), n).evaluate(zeta)
    az, bz, cz = proof["a_s_poly_zeta"], proof["b_s_poly_zeta"], proof["c_s_poly_zeta"]
    zwz, s1z, s2z = proof["w_accumulator_poly_zeta"], proof["sigma1_poly_zeta"], proof["sigma2_poly_zeta"]
    a2 = alpha * alpha % R
    r0 = (pi_zeta - l1 * a2 - alpha * ((az + s1z * beta + gamma) * (bz + s2z * beta + gamma) % R * (cz + gamma) % R * zwz)) % R
    k_acc = ((az + zeta * beta + gamma) * (bz + 2 * zeta * beta + gamma) % R * (cz + 3 * zeta * beta + gamma) % R * alpha + l1 * a2 + mu) % R
    k_s3 = (az + s1z * beta + gamma) * (bz + s2z * beta + gamma) % R * alpha % R * beta % R * zwz % R
    es = (nu * az + pow(nu, 2, R) * bz + pow(nu, 3, R) * cz + pow(nu, 4, R) * s1z + pow(nu, 5, R) * s2z + mu * zwz - r0) % R
    t = [az * bz, az, bz, cz, 1, pow(nu, 4, R), pow(nu, 5, R), -k_s3, nu, pow(nu, 2, R), pow(nu, 3, R), k_acc,
         -zh, -zh * zn, -zh * zn * zn, zeta, w * mu * zeta, -es, 1, mu]
    return [x % R for x in t]


def test_scalar_table_under_asan_and_ubsan_equals_the_model(tmp_path):
    exe = str(tmp_path / "plonk_scalars_sanitize")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "plonk_scalars_sanitize.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=120)
    out, err = p.stdout.decode(), p.stderr.decode()
    assert p.returncode == 0, (out[-2000:], err[-4000:])
    assert "runtime error" not in err and "AddressSanitizer" not in err and "LeakSanitizer" not in err, err[-4000:]
    assert out.strip().endswith("ok")
    n, tau = 8, 19
    cpi, wit = PL.random_circuit(n, random.Random(8), random.Random(1008))
    rng = random.Random(4)
    proof = PL.prove(cpi, wit, tau, [rng.randrange(R) for _ in range(11)], n_srs=4 * n + 1)
    zeta = PL.compute_verifier_challenges(proof)[3]
    want = model_table(n, proof, PL.to_coefficient_poly(wit["public_poly"], n).evaluate(zeta))
    got = [int(line.split()[2], 16) for line in out.splitlines() if line.startswith("term")]
    assert got == want
    # the table is the model's verifier: summing scalar * point over it gives verifier_points' pair
    v = PL.vpi(cpi, tau)
    pts = [v[f] for f in PL.CPI_FIELDS] + [proof[f] for f in PL.POINT_FIELDS] + [M.G1, proof["w_zeta_commitment"], proof["w_zeta_omega_commitment"]]
    right = PL._msm(zip(pts[:18], want[:18]))
    left = PL._msm(zip(pts[18:], want[18:]))
    assert (left, right) == PL.verifier_points(n, proof, v, wit["public_poly"])
