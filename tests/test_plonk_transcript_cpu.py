"""The Fiat-Shamir schedule every PLONK entry point shares (csrc/plonk_transcript.hpp, host only: the Merlin transcript, the decimal
printer of a point, PlonkRoundTranscript) under g++ -fsanitize=address,undefined, as a stand-alone program
(tests/cpp/plonk_transcript_sanitize.cpp).  The program reads proofs from standard input and prints their six challenges; this test
compares them with plonk_model.compute_verifier_challenges on the same data.  The transcript checks no curve membership, so the
coordinates aim at the printer: canonical 0 (ark prints the empty string), 1, 10^19 - 1 and 10^19 (the printer divides by 10^19), 10^38
(an all-zero middle chunk) and p - 1, with a point at infinity in every round's group."""
import os
import random
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import plonk_model as PL  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M, R = PL.M, PL.R
P = M.P
POINTS = PL.POINT_FIELDS                            # the ABI's order of the nine points
EVALS = PL.PROOF_FIELDS[7:13]                       # and of the six evaluations
EDGES = [0, 1, 10 ** 19 - 1, 10 ** 19, 10 ** 38, P - 1]


def words(value, count, modulus):
    """`count` 64-bit words of value's Montgomery form, least significant first"""
    mont = value * pow(2, 64 * count, modulus) % modulus
    return ["%x" % ((mont >> (64 * i)) & (2 ** 64 - 1)) for i in range(count)]


def serialise(proof):
    out = []
    for f in POINTS:
        x, y = proof[f] if proof[f] is not None else (0, 0)
        out += words(x, 6, P) + words(y, 6, P)
    out += ["1" if proof[f] is None else "0" for f in POINTS]
    for f in EVALS:
        out += words(proof[f], 4, R)
    return " ".join(out)


def edge_proof(shift, infinite, evals):
    """point i is (EDGES[i + shift], EDGES[i + shift + 1]) cyclically, the identity where i is in `infinite`"""
    proof = {f: None if i in infinite else (EDGES[(i + shift) % 6], EDGES[(i + shift + 1) % 6]) for i, f in enumerate(POINTS)}
    proof.update(zip(EVALS, evals))
    return proof


def proofs():
    rng = random.Random(2024)
    n, tau = 4, 19
    cpi, wit = PL.random_circuit(n, random.Random(5), random.Random(1005))
    real = PL.prove(cpi, wit, tau, [rng.randrange(R) for _ in range(11)], n_srs=4 * n + 1)
    # the groups of the rounds are points 0-2, 3, 4-6 and 7-8: one identity in each, then none, then the other members
    return [real,
            edge_proof(0, {1, 3, 5, 8}, [0, 1, R - 1] + [rng.randrange(R) for _ in range(3)]),
            edge_proof(1, set(), [rng.randrange(R) for _ in range(6)]),
            edge_proof(3, {0, 2, 4, 6, 7}, [rng.randrange(R) for _ in range(3)] + [R - 1, 0, 1])]


def test_every_edge_coordinate_is_both_an_x_and_a_y():
    seen_x, seen_y = set(), set()
    for p in proofs()[1:]:
        for f in POINTS:
            if p[f] is not None:
                seen_x.add(p[f][0])
                seen_y.add(p[f][1])
    assert seen_x == set(EDGES) and seen_y == set(EDGES)


def test_challenges_under_asan_and_ubsan_equal_the_model(tmp_path):
    exe = str(tmp_path / "plonk_transcript_sanitize")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "plonk_transcript_sanitize.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    all_proofs = proofs()
    text = "\n".join(serialise(p) for p in all_proofs).encode()
    outs = []
    for _ in range(2):                              # the same input twice: nothing of a run may depend on what memory held
        p = subprocess.run([exe], input=text, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=120)
        out, err = p.stdout.decode(), p.stderr.decode()
        assert p.returncode == 0, (out[-2000:], err[-4000:])
        assert "runtime error" not in err and "AddressSanitizer" not in err and "LeakSanitizer" not in err, err[-4000:]
        assert out.strip().endswith("ok %d" % len(all_proofs))
        outs.append(out)
    assert outs[0] == outs[1]
    got = [tuple(int(w, 16) for w in line.split()[1:]) for line in outs[0].splitlines() if line.startswith("challenges")]
    want = [PL.compute_verifier_challenges(p) for p in all_proofs]
    assert got == want
    # gamma follows beta with nothing absorbed between them, so it is one constant; every other challenge depends on its proof
    assert len({c for row in got for c in row}) == 5 * len(all_proofs) + 1
