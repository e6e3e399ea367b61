"""Adversarial inputs for the bucket-method MSM (csrc/msm_kernels.hpp) and what its stages must make of them, in plain Python:
the signed-digit recoding restated, scalar families aimed at the digit boundaries, bucket populations aimed at the heavy-bucket
thresholds, the expected sort state and heavy filing, and the exponent of a commitment.  Imports neither the oracle nor the package."""
import numpy as np

R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
HEAVY_REC = 2048        # points per level-0 record
HEAVY_FAN = 256         # partial sums per record of the levels above
COUNT_CLAMP = 1023      # the order pass sorts the buckets by min(count, 1023)
# the sizes the GPU files run and the CPU file checks the inputs for: one list each
PLAIN_SIZES = [1, 63, 300, 512, 2047, 2048, 2049, 4047, 4096, 4097, 5000, 1 << 13, 14436, 1 << 14, 1 << 16, 1 << 20, 1050659]
BATCHES = [[0, 1, 299, 4999, 16383], list(range(0, 5 * 64 + 1, 5))]          # problem offsets from 0
TABLES = [(1, 1), (63, 63), (64, 64), (65, 65), (100, 256), (300, 300), (4095, 4095), (4096, 4096), (5000, 5000), (1 << 13, 1 << 13),
          (1 << 14, 1 << 14), (1 << 15, 1 << 15), (1 << 16, 1 << 16), (5000, 1 << 16), (1 << 20, 1 << 20)]      # (scalars, SRS points)
LEVEL_VARS = [8, 12, 13, 16, 20]                                               # openings of 2^n_vars entries
DIGIT_SIZES = [1, 300, 4096, 5000, 1 << 13, 1 << 16, 1 << 20]                  # the digit sweep's geometries (a subset of the above)
POPULATION_COUNTS = [1, 2, "heavy_min-1", "heavy_min", "heavy_min+1", 2047, 2048, 2049, 4096, 4097]


# ---- the recoding rule: low window first; raw = low c bits + carry; raw > 2^(c-1): digit raw - 2^c, carry 1; else digit raw, carry 0 ----
def recode(s, widths):
    """-> (digits, carries, final carry): carries[w] is the carry OUT of window w"""
    digits, carries, carry = [], [], 0
    for c in widths:
        raw = (s & ((1 << c) - 1)) + carry
        s >>= c
        if raw > (1 << (c - 1)):
            digits.append(raw - (1 << c))
            carry = 1
        else:
            digits.append(raw)
            carry = 0
        carries.append(carry)
    return digits, carries, carry


def levels_of(n_vars):
    """the problems of an opening of 2^n_vars entries: its rounds, 2^(n_vars - 1) ... 1 quotient entries, as offsets"""
    out = [0]
    for k in range(n_vars - 1, -1, -1):
        out.append(out[-1] + (1 << k))
    return out


def bit_offsets(widths):
    out, bit = [], 0
    for c in widths:
        out.append(bit)
        bit += c
    return out


def reconstruct(digits, widths):
    return sum(d << b for d, b in zip(digits, bit_offsets(widths)))


def digits_np(scalars, widths):
    """the same rule over many scalars at once -> int64 [n, len(widths)]"""
    n = len(scalars)
    raw = np.frombuffer(b"".join(int(s).to_bytes(40, "little") for s in scalars), dtype=np.uint8).reshape(n, 40)
    bits = np.unpackbits(raw, axis=1, bitorder="little")
    out = np.empty((n, len(widths)), dtype=np.int64)
    carry = np.zeros(n, dtype=np.int64)
    for w, (c, b) in enumerate(zip(widths, bit_offsets(widths))):
        val = bits[:, b: b + c].astype(np.int64) @ (np.int64(1) << np.arange(c, dtype=np.int64)) + carry
        neg = val > (1 << (c - 1))
        out[:, w] = val - (neg.astype(np.int64) << c)
        carry = neg.astype(np.int64)
    assert not carry.any()
    return out


def uniform_widths(c):
    """256 bits in windows of c bits: ceil(256 / c) of them where that stays within the 264 bits the digit launcher takes, else
    floor(256 / c) with the bits left added to the top window (exactly 256 bits; the top window stays below 32 bits)"""
    w = (256 + c - 1) // c
    if w * c <= 264:
        return [c] * w
    return [c] * (256 // c - 1) + [c + 256 % c]


# ---- scalar families, each built from a list of window widths and each canonical (< r) ---------------------------------------------------
def _lower(widths, digit_of):
    """sum over the windows below the top of digit_of(c) 2^(first bit)"""
    return sum(digit_of(c) << b for c, b in list(zip(widths, bit_offsets(widths)))[:-1])


def _fit_top(lower, widths, want):
    """lower + t 2^(first bit of the top window) with the largest 0 <= t <= want that is canonical and recodes without a final carry"""
    top = bit_offsets(widths)[-1]
    t = min(want, (R - 1 - lower) >> top)
    while t >= 0:
        s = lower + (t << top)
        if s < R and recode(s, widths)[2] == 0:
            return s
        t -= 1
    raise AssertionError("no canonical top window")


def half(widths):
    return _fit_top(_lower(widths, lambda c: 1 << (c - 1)), widths, 1 << (widths[-1] - 1))


def half_plus_one(widths):
    return half(widths) + 1


def ones_run(widths):
    return (1 << bit_offsets(widths)[-1]) - 1


def all_equal(widths, d):
    return _fit_top(_lower(widths, lambda c: d), widths, d)


def top_heavy(widths):
    """r - 1 - k for k = 1, 2, 3, and the two sides of the carry into the top window at its largest value T = (r - 1) >> first bit:
    the largest scalar with top window T that does not carry into it, and (where canonical) the smallest that does"""
    top = bit_offsets(widths)[-1]
    T, L = (R - 1) >> top, (R - 1) & ((1 << top) - 1)
    hl = _lower(widths, lambda c: 1 << (c - 1))
    out = [R - 2, R - 3, R - 4, (T << top) | min(L, hl)]
    if hl + 1 <= L:
        out.append((T << top) | (hl + 1))
    return out


def families(widths):
    """name -> list of scalars"""
    c_min = min(widths)
    return {"half": [half(widths)], "half_plus_one": [half_plus_one(widths)], "ones_run": [ones_run(widths)],
            "all_equal_1": [all_equal(widths, 1)], "all_equal_2": [all_equal(widths, min(2, 1 << (c_min - 1)))],
            "all_equal_half": [all_equal(widths, 1 << (c_min - 1))], "minus_one": [R - 1], "top_heavy": top_heavy(widths)}


def family_scalars(widths):
    return [s for v in families(widths).values() for s in v]


def uniform(n, seed):
    """n seeded uniform canonical scalars"""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        v = int.from_bytes(rng.bytes(32), "little") >> 1
        if v < R:
            out.append(v)
    return out


_MONT = {}


def to_mont(scalars):
    """canonical ints -> uint64 [n, 4] stored (Montgomery) limbs, what the kernels read"""
    cache, rows = _MONT, []
    if len(cache) > (1 << 18):
        cache.clear()
    for s in scalars:
        if s not in cache:
            m = s * (1 << 256) % R
            cache[s] = [(m >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(4)]
        rows.append(cache[s])
    return np.array(rows, dtype=np.uint64).reshape(len(rows), 4)


_POOL = []


def _uniform_pool(count):
    """the first `count` scalars of one seeded uniform stream (generated once, extended on demand)"""
    if len(_POOL) < count:
        _POOL[:] = uniform(max(count, 1 << 12), 4242)
    return _POOL[:count]


def cycled(pool, n, seed, mix=False):
    """the pool's scalars cycled over n positions by a seeded permutation; mix: every other position a uniform scalar instead"""
    rng = np.random.default_rng(seed)
    perm = rng.permutation(n)
    out = [0] * n
    uni = _uniform_pool(n // 2 + 1) if mix else None
    for k, p in enumerate(perm):
        out[int(p)] = uni[k // 2] if (mix and k & 1) else pool[k % len(pool)]
    return out


# ---- bucket populations at the filing thresholds -----------------------------------------------------------------------------------------
def population_values(c0, how_many):
    """window-0 digit values: the last two buckets (first, so that the smallest case populates them), the first two, the segment edge
    (8, 9), the partition edge (256, 257); two more partition edges (255, 512) when every count of POPULATION_COUNTS is placed"""
    h = 1 << (c0 - 1)
    vals = []
    for v in [h, h - 1, 1, 2, 8, 9, 256, 257, 255, 512]:
        if 1 <= v <= h and v not in vals:
            vals.append(v)
    return vals[:how_many]


def population_counts(n, heavy_min, n_values):
    """the longest prefix of the counts (ascending) that fits n points and the values at hand"""
    out = []
    for c in POPULATION_COUNTS:
        c = {"heavy_min-1": heavy_min - 1, "heavy_min": heavy_min, "heavy_min+1": heavy_min + 1}.get(c, c)
        if sum(out) + c <= n and len(out) < n_values:
            out.append(c)
    return out


def population(n, widths, heavy_min, seed, avoid_all_windows=False):
    """-> (scalars, {value: count}).  A seeded permutation of the positions places count copies of the small scalar v (one digit: v in
    window 0); the positions left get uniform scalars whose window-0 digit (every digit with avoid_all_windows: the shared bucket set of
    a table) has none of the placed magnitudes.  Bucket v - 1 of window 0 then holds exactly count points."""
    vals = population_values(widths[0], len(POPULATION_COUNTS))
    counts = population_counts(n, heavy_min, len(vals))
    placed = dict(zip(vals, counts))
    rng = np.random.default_rng(seed)
    perm = [int(p) for p in rng.permutation(n)]
    out, k = [None] * n, 0
    for v, c in placed.items():
        for p in perm[k: k + c]:
            out[p] = v
        k += c
    mags, seed2 = set(placed), seed + 1000
    while k < n:
        for s in uniform(n - k, seed2):
            d = recode(s, widths)[0]
            if not any(abs(x) in mags for x in (d if avoid_all_windows else d[:1])):
                out[perm[k]] = s
                k += 1
        seed2 += 1
    return out, placed


# ---- the expected sort state and heavy filing --------------------------------------------------------------------------------------------
def expected_sort(scalars, geo, inf=None):
    """geo: msm_driver.Geometry.  -> (counts uint32 [n_buckets], keys): keys = the (bucket << 32 | entry) of every (point, window) pair
    with a non-zero digit, ascending; entry = (entry_off + i) | sign << 31, i the point's index in the pass"""
    counts = np.zeros(geo.n_buckets, dtype=np.int64)
    keys = []
    for j in range(geo.n_problems):
        lo, hi = geo.offsets[j], geo.offsets[j + 1]
        if hi == lo:
            continue
        widths = geo.widths(j)
        dig = digits_np(scalars[lo:hi], widths)
        idx = np.arange(lo, hi, dtype=np.int64)
        live = np.ones(hi - lo, dtype=bool) if inf is None else (np.asarray(inf[lo:hi]) == 0)
        for w in range(len(widths)):
            _, set_idx, entry_off = geo.wins[geo.win_first[j] + w]
            c_set, bucket_base, _, _ = geo.sets[set_idx]
            d = dig[:, w]
            m = live & (d != 0)
            mag = np.abs(d[m])
            assert (mag <= (1 << (c_set - 1))).all()
            bucket = bucket_base + mag - 1
            entry = ((entry_off + idx[m]) & 0x7FFFFFFF) | ((d[m] < 0).astype(np.int64) << 31)
            assert ((entry_off + idx[m]) & 0xFFFFFFFF < (1 << 31)).all()
            counts += np.bincount(bucket, minlength=geo.n_buckets)
            keys.append((bucket << 32) | entry)
    keys = np.sort(np.concatenate(keys)) if keys else np.zeros(0, dtype=np.int64)
    return counts.astype(np.uint32), keys


def filing(cnt):
    """how msm_file_heavy files a heavy bucket of cnt points -> (records per level [4], level of the final record, slots used)"""
    groups = (cnt + HEAVY_REC - 1) // HEAVY_REC
    if groups == 1:
        return [1, 0, 0, 0], 0, 0
    n_rec, slots, count = [groups, 0, 0, 0], groups, groups
    for level in (1, 2, 3):
        groups = (count + HEAVY_FAN - 1) // HEAVY_FAN
        if groups == 1:
            n_rec[level] += 1
            return n_rec, level, slots
        n_rec[level] += groups
        slots += groups
        count = groups
    raise AssertionError("more than 2^27 points in one bucket")


def expected_overflow(counts, heavy_min):
    """-> (n_slots, n_rec[4], {bucket: final level}) over the buckets holding more than heavy_min points"""
    n_rec, slots, final = [0, 0, 0, 0], 0, {}
    for b in np.nonzero(counts > heavy_min)[0]:
        r, level, s = filing(int(counts[b]))
        n_rec = [a + x for a, x in zip(n_rec, r)]
        slots += s
        final[int(b)] = level
    return slots, n_rec, final


# ---- the closed form of a commitment -------------------------------------------------------------------------------------------------------
def exponent(scalars, logs, skip=()):
    """sum s_i k_i mod r, k_i the discrete logarithm of SRS point i (the indices in `skip` are points at infinity)"""
    acc = 0
    for i, (s, k) in enumerate(zip(scalars, logs)):
        if i not in skip:
            acc += s * k
    return acc % R


def univariate_logs(tau, n):
    out, k = [], 1
    for _ in range(n):
        out.append(k)
        k = k * tau % R
    return out


def eq_log(tau, i):
    """eq_i(tau), MSB first: the discrete logarithm of point i of a multilinear SRS"""
    nv, acc = len(tau), 1
    for b in range(nv):
        t = tau[b]
        acc = acc * (t if (i >> (nv - 1 - b)) & 1 else 1 - t) % R
    return acc


def mle_eval(table, point):
    """the multilinear extension of `table` at `point`, first variable = most significant index bit"""
    t = list(table)
    for z in point:
        h = len(t) // 2
        t = [(t[k] + z * (t[h + k] - t[k])) % R for k in range(h)]
    return t[0]


def spot_indices(n, seed):
    rng = np.random.default_rng(seed)
    return sorted({i for i in [0, 1, 2047, 2048, n - 1, int(rng.integers(0, n)), int(rng.integers(0, n))] if 0 <= i < n})
