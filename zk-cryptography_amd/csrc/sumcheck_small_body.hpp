// sumcheck_small_body.hpp -- NOT a header: the body of sumcheck_small_kernel (multifold_kernels.hpp, which describes it), as text.
// It is included inside that kernel and inside workgroup 0 of fold_rounds_kernel (fold_rounds.hpp); in scope where it is included:
//     SmallArgs a, SumcheckDev* st, uint64_t* __restrict__ round_polys, uint64_t* __restrict__ challenges
// and nothing else of the includer: it declares the dynamic LDS (zk_dyn_lds, an extern redeclared where the includer has it already) and
// every local itself, so it goes into a block of its own; it contains the workgroup's barriers and assumes SMALL_BLOCK lanes.
// Text and not a __device__ function: behind a shared function -- arguments by value or by reference, the LDS declared inside or handed
// in -- the stand-alone kernel kept its register counts but not its code (another allocation, 2706 lines of assembly differ), and it
// runs in every proof.  As text it is the same token sequence as before inside the same kernel: tools/device_asm_diff.py reads identical.
    extern __shared__ __attribute__((aligned(16))) unsigned char zk_dyn_lds[];
    __builtin_amdgcn_s_setprio(3);                      // the chip's critical path: win every issue arbitration
    ZK_STAMP_AT(0, 40 + a.round0, 0);                   // diagnostics: kernel entry
    const uint32_t n = 1u << a.log_n;
    Fr* tree0 = reinterpret_cast<Fr*>(zk_dyn_lds);      // 2n nodes, canonical values
    Fr* tree1 = tree0 + 2 * n;                          // n nodes: the first tree built here is already a folded one
    // weights (Montgomery), ping / pong: 2^(it+1) of them after round it, so the array that receives the last round's
    // holds 2^n_rounds and the other one half of that; no region at all when none are asked for
    const uint32_t w_all = a.weights_out ? (1u << a.n_rounds) : 0u;
    Fr* w0 = tree1 + n;
    Fr* w1 = w0 + ((a.n_rounds & 1) ? w_all / 2 : w_all);
    const bool grouped = a.group != 0 && a.stride == 0;
    Fr* scratch = w0 + w_all + w_all / 2 + 1;           // SMALL_BLOCK entries, only in the grouped mode
    Fr* e_sh = scratch + (grouped ? SMALL_BLOCK : 0);   // 2: to_mont(level-2 differences) of tree0, for the first round's product
    // ---- leaves (sums are taken as they come -- the conversion to canonical integers is linear -- then converted once)
    if (a.group == 0) {
        for (uint32_t j = threadIdx.x; j < n; j += SMALL_BLOCK) {
            const Fr v = load_fr(a.src, j);
            tree0[n + j] = a.canon ? v : fr_from_mont_outlined(v);
        }
    } else if (a.stride != 0) {   // partial tables (blockfold_kernel's term ranges, or all-gathered per-rank block sums in rank order)
        for (uint32_t j = threadIdx.x; j < n; j += SMALL_BLOCK) {
            // every partial of an entry in ONE batch of 8 loads (the serial kernel's prologue is latency; blockfold_kernel leaves <= 8
            // tables).  No load hangs on a branch: a slot past the last partial reads the last one again and is not added.
            Fr s;
            for (uint32_t g = 0; g < a.group; g += 8) {
                Fr v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const uint32_t gu = g + u < a.group ? g + u : a.group - 1;
                    v[u] = load_fr(a.src, (size_t)gu * a.stride + j);
                }
                if (g == 0) s = v[0];
#pragma unroll
                for (int u = 0; u < 8; ++u) if (g + u < a.group && g + u != 0) s = s + v[u];
            }
            tree0[n + j] = a.canon ? s : fr_from_mont_outlined(s);
        }
    } else {
        const uint32_t total = n * a.group;
        const uint32_t run = total > (uint32_t)SMALL_BLOCK ? total / SMALL_BLOCK : 1;   // consecutive partials per thread
        if (threadIdx.x * run < total) {
            Fr s = Fr::zero();
            for (uint32_t g = 0; g < run; ++g) s = s + load_fr(a.src, (size_t)threadIdx.x * run + g);
            scratch[threadIdx.x] = s;
        }
        __syncthreads();
        const uint32_t tpe = a.group / run;   // scratch slots per entry (run <= group because n <= SMALL_BLOCK in this mode)
        for (uint32_t j = threadIdx.x; j < n; j += SMALL_BLOCK) {
            Fr s = scratch[j * tpe];
            for (uint32_t g = 1; g < tpe; ++g) s = s + scratch[j * tpe + g];
            tree0[n + j] = a.canon ? s : fr_from_mont_outlined(s);
        }
    }
    if (threadIdx.x == 0 && a.weights_out) {
        Fr one32;   // Montgomery form of 2^32: the k-variable fold reduces with 9 words instead of 8
        constexpr uint32_t c[8] = {0xcaaf6b13u, 0x355094eau, 0x69a568efu, 0xf6b10cb3u, 0x40cc3869u, 0xe2c926a6u, 0xed269aadu, 0x736a6d3bu};
#pragma unroll
        for (int i = 0; i < 8; ++i) one32.l[i] = c[i];
        w0[0] = one32;
    }
    __syncthreads();
    // ---- inner levels, bottom up, three levels per barrier: a lane sums the subtree under 8 nodes of the level below
    for (uint32_t lvl = a.log_n; lvl > 1;) {
        const uint32_t step = lvl - 1 < 3 ? lvl - 1 : 3;
        const uint32_t groups = 1u << (lvl - step);
        for (uint32_t g = threadIdx.x; g < groups; g += SMALL_BLOCK) {
            Fr v[8];
            const uint32_t cnt0 = 1u << step;
#pragma unroll
            for (int i = 0; i < 8; ++i) if ((uint32_t)i < cnt0) v[i] = tree0[(1u << lvl) + g * cnt0 + i];
#pragma unroll
            for (int sft = 1; sft <= 3; ++sft) {
                if ((uint32_t)sft <= step) {
                    const uint32_t cnt = cnt0 >> sft;
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        if ((uint32_t)i < cnt) {
                            v[i] = v[2 * i] + v[2 * i + 1];
                            tree0[(1u << (lvl - sft)) + g * cnt + i] = v[i];
                        }
                    }
                }
            }
        }
        __syncthreads();
        lvl -= step;
    }
    // ---- rounds.  Every round hashes the same two-block message from the initial hash value:
    //   block 1 = prefix (the previous challenge's digest; in the first round of a proof the claimed sum) || lo
    //   block 2 = hi || 0x80 padding || length (96 bytes)
    // (commit(lo), commit(hi), challenge() of fiat_shamir.rs:17-25 after a challenge() has re-seeded the hasher).
    // Wave 0 runs the rounds of the two compressions; wave 1 prepares the schedule of block 1, wave 2 that of block 2
    // (sha256_schedule_to_lds), both from their own copy of lo / hi, one round ahead of the hash.
    const uint32_t wave = threadIdx.x >> 6;
    const bool wave0 = wave == 0;
    uint32_t* kw1 = reinterpret_cast<uint32_t*>(e_sh + 2);      // 64 words
    uint32_t* kw2 = kw1 + 64;                                   // 64 words
    uint32_t* dig_sh = kw2 + 64;                                // 2 x 8: raw digest of the last challenge, double-buffered
    uint32_t* flags = dig_sh + 16;                              // [0]: kw1 progress, [1]: kw2 progress (+ 2 words of padding)
    uint32_t* aff_sh = flags + 4;                               // 2 x 2 tables of digit multiples (affine_step.hpp), double-buffered
    Fr* aff_stage = reinterpret_cast<Fr*>(aff_sh + 4 * AFF_TABLE_WORDS);   // 2 x 10: the builders' X * 2^(28 k), one wave's own exchange
    if (threadIdx.x >= 64 && threadIdx.x < 66 && a.log_n >= 2)
        e_sh[threadIdx.x - 64] = (tree0[6 + threadIdx.x - 64] - tree0[4 + threadIdx.x - 64]).to_mont();
    if (threadIdx.x == 0) {
        flags[0] = 0; flags[1] = 0;
        // prefix of the first round run here
        uint32_t pre[8];
        if (a.first) {
            const Fr sum_c = (a.first == 2) ? fr_from_mont_outlined(fr_from_arg(a.claimed))
                           : (a.first == 3) ? fr_from_mont_outlined(load_fr(a.d_claimed, 0)) : tree0[2] + tree0[3];
#pragma unroll
            for (int i = 0; i < 8; ++i) pre[i] = sum_c.l[7 - i];
        } else {   // a kernel always stops after a challenge(): initial hash value, the digest pending
#pragma unroll
            for (int i = 0; i < 8; ++i) pre[i] = st->transcript.buf[i];
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) dig_sh[8 + i] = pre[i];     // slot (it - 1) & 1 for it = 0
    }
    __syncthreads();
    // the round polynomial's lo (canonical) as the hash wave keeps it: limbs in registers that no lane-indexed read ever touches (an
    // element read through fr_limb_by_lane lives in scratch, and a round trip through scratch per round was on the path)
    uint32_t low[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) low[i] = tree0[2].l[i];
    uint32_t depth = a.log_n, round = a.round0, n_w = 1;
    ZK_STAMP_AT(0, 40 + a.round0, 1);                   // prologue done
    // schedules of round 0 (waves 1 and 2)
    // (a word per lane: lane i of every row holds word i of the block -- sha256_schedule_rows_to_lds)
    const uint32_t word = threadIdx.x & 15;
    // (lo_w: lanes 8 .. 15 of a row hold limb 15 - word of lo; hi_w: lanes 0 .. 7 hold limb 7 - word of hi)
    auto schedule_block1_words = [&](const uint32_t* prefix, uint32_t lo_w, uint32_t it) {
        const uint32_t w = word < 8 ? prefix[word] : lo_w;
        sha256_schedule_rows_to_lds(w, kw1, flags, 4 * it, 1, threadIdx.x < 64 + 16);
    };
    auto schedule_block2_words = [&](uint32_t hi_w, uint32_t it) {
        const uint32_t w = word < 8 ? hi_w : (word == 8 ? 0x80000000u : word == 15 ? 96u * 8u : 0u);
        sha256_schedule_rows_to_lds(w, kw2, flags + 1, 4 * it, 0, threadIdx.x < 128 + 16);
    };
    auto schedule_block1 = [&](const uint32_t* prefix, const Fr& lo_c, uint32_t it) {
        schedule_block1_words(prefix, fr_limb_by_lane(lo_c, 15 - word), it);
    };
    auto schedule_block2 = [&](const Fr& hi_c, uint32_t it) { schedule_block2_words(fr_limb_by_lane(hi_c, 7 - word), it); };
    AffineLane aff;                                     // this lane's limb of r and of 2^256 - r, for the rounds' closing step
    aff.init();
    // The table builders: lanes of the last helper wave, per value (lo', hi': b_v2) and digit (b_k) one lane of each half wave.  The
    // first half's lanes take the part of the table that waits for the challenge, the second half's the part that does not; every
    // builder keeps its one constant (a power of 2^28 in the Montgomery form its part needs) in registers for the whole launch.
    const uint32_t bl = threadIdx.x - (SMALL_BLOCK - 64);
    const bool builder = bl < 64 && (bl & 31) < 2 * AFF_DIGITS;
    const uint32_t b_free = bl >> 5, b_v2 = (bl & 31) >= (uint32_t)AFF_DIGITS ? 1u : 0u, b_k = (bl & 31) - AFF_DIGITS * b_v2;
    const Fr b_pow = affine_pow_mont(builder ? b_k + AFF_DIGITS * (1 - b_free) : 0u);
    if (a.n_rounds) {
        if (wave == 1) schedule_block1_words(dig_sh + 8, tree0[2].l[(15 - word) & 7], 0);
        if (wave == 2) schedule_block2_words(tree0[3].l[(7 - word) & 7], 0);
    }
    uint32_t digest[8];
    // Waves 3, 5, 6, 7 fold the trees and the weights.  Wave 4 sits on the transcript wave's SIMD (waves go round the four SIMDs),
    // where every instruction it issues is one the hash waits for: it only records the round's outputs, which nobody in this
    // kernel reads, and at the lowest priority.
    constexpr uint32_t FIRST_HELPER = 192, N_HELPERS = SMALL_BLOCK - FIRST_HELPER - 64, OUT_WAVE = 4;
    if (wave == OUT_WAVE) {
        __builtin_amdgcn_s_setprio(0);
        // what earlier kernels of this proof recorded -- sum, round polynomials and challenges of rounds < round0 -- goes to the pinned
        // mirror from here: no wave on the path issues these stores (they cross PCIe) or waits behind them
        if (a.host_delta && a.round0) {
            for (uint32_t i = threadIdx.x - 64 * OUT_WAVE; i < 12 * a.round0 + 4; i += 64) {
                const uint64_t* p = i < 4 ? st->sum + i : i < 4 + 8 * a.round0 ? round_polys + (i - 4) : challenges + (i - 4 - 8 * a.round0);
                *const_cast<uint64_t*>(p + a.host_delta) = *p;
            }
        }
    }
    for (uint32_t it = 0; it < a.n_rounds; ++it) {
        Fr* told = (it & 1) ? tree1 : tree0;
        Fr* tnew = (it & 1) ? tree0 : tree1;
        Fr* wold = (it & 1) ? w1 : w0;
        Fr* wnew = (it & 1) ? w0 : w1;
        // the tables of digit multiples of this round's level-2 differences were built a round ago (never for the first round here)
        uint32_t* tbl_old = aff_sh + 2 * AFF_TABLE_WORDS * (it & 1);
        uint32_t* tbl_new = aff_sh + 2 * AFF_TABLE_WORDS * ((it & 1) ^ 1);
        const bool tabled = it != 0;
        const bool absorb_sum = a.first && it == 0;
        if (wave0) {
            ZK_STAMP_AT(0, round, 0);
            uint32_t h[8] = {0x6a09e667u, 0xbb67ae85u, 0x3c6ef372u, 0xa54ff53au, 0x510e527fu, 0x9b05688cu, 0x1f83d9abu, 0x5be0cd19u};
            uint32_t blk[16];
            const uint32_t* pre = dig_sh + 8 * ((it + 1) & 1);
#pragma unroll
            for (int i = 0; i < 8; ++i) { blk[i] = pre[i]; blk[8 + i] = low[7 - i]; }
            ShaSplit sp;                                              // the state rounds on six lanes (transcript.hpp)
            sp.init();
            uint32_t hs[4];
            sp.split(h, hs);
            sha256_compress_kw_split(sp, hs, blk, kw1, flags, 4 * it);          // uni_poly.to_bytes()  sumcheck.rs:42
            ZK_STAMP_AT(0, round, 1);
            sha256_compress_kw_split(sp, hs, nullptr, kw2, flags + 1, 4 * it);  // challenge()  :46
            sp.join(hs, h);
            ZK_STAMP_AT(0, round, 2);
#pragma unroll
            for (int i = 0; i < 8; ++i) digest[i] = h[i];
            if (threadIdx.x == 0) {   // the raw digest: whoever needs the challenge (from_be_bytes_mod_order) reduces it for itself
#pragma unroll
                for (int i = 0; i < 8; ++i) dig_sh[8 * (it & 1) + i] = h[i];
            }
        }
        ZK_STAMP_AT(0, round, 3);
        ZK_STAMP_AT(SMALL_BLOCK - 1, round, 6);      // the last helper -- the wave that builds the tables -- arrives at the barrier
        ZK_STAMP_AT(64, round, 7);                   // the first schedule wave arrives
        __syncthreads();   // digest published; tree `told` and the tables `tbl_old` complete
        ZK_STAMP_AT(0, round, 4);
        // the digest as an integer (little-endian limbs): wave 0 has it in registers, everybody else reads the slot
        uint32_t dl[8];
        if (wave0) {
#pragma unroll
            for (int i = 0; i < 8; ++i) dl[i] = digest[7 - i];
        } else {
#pragma unroll
            for (int i = 0; i < 8; ++i) dl[i] = dig_sh[8 * (it & 1) + 7 - i];
        }
        auto challenge_canonical = [&]() {
            Fr c;
#pragma unroll
            for (int i = 0; i < 8; ++i) c.l[i] = dl[i];
            c.reduce_once();
            c.reduce_once();
            return c;
        };
        if (wave <= 2) {
            // Next round polynomial straight from level 2 of the old tree: lo' = t[4] + c * (t[6] - t[4]), hi' likewise from t[5], t[7].
            // Wave 0 (the next block 1's words 8 .. 15) and wave 1 (its schedule) take lo', wave 2 hi' (block 2's schedule; its hash is
            // already waiting for them).  One limb per lane from the table (affine_step.hpp); the first round of a launch, which has no
            // table, multiplies as before.
            const uint32_t q = wave == 2 ? 1u : 0u;
            if (depth >= 2 && (wave0 || it + 1 < a.n_rounds)) {
                if (tabled) {
                    uint32_t dg[AFF_DIGITS];
                    affine_digits(dl, dg);
                    const uint32_t limb = affine_step_rows(aff, told[4 + q].l[word & 7], tbl_old + AFF_TABLE_WORDS * q, dg);
                    if (wave0) {
#pragma unroll
                        for (int i = 0; i < 8; ++i) low[i] = __builtin_amdgcn_readlane(limb, i);
                    } else if (wave == 1) {
                        schedule_block1_words(dig_sh + 8 * (it & 1), aff_row_mirror(limb), it + 1);
                    } else {
                        schedule_block2_words(aff_row_half_mirror(limb), it + 1);
                    }
                } else {
                    const Fr v = told[4 + q] + fr_mul_outlined(challenge_canonical(), e_sh[q]);
                    if (wave0) {
#pragma unroll
                        for (int i = 0; i < 8; ++i) low[i] = v.l[i];
                    } else {
                        const Fr vs = v;                             // the copy the lane-indexed reads go to
                        if (wave == 1) schedule_block1(dig_sh + 8 * (it & 1), vs, it + 1);
                        else schedule_block2(vs, it + 1);
                    }
                }
            }
            if (wave0) ZK_STAMP_AT(0, round, 5);
        } else {
            const Fr c = challenge_canonical();
            const uint32_t helper = wave == OUT_WAVE ? N_HELPERS : wave < OUT_WAVE ? threadIdx.x - FIRST_HELPER : threadIdx.x - FIRST_HELPER - 64;
            const uint32_t nodes = 1u << (depth - 1);   // the new tree has nodes 1 .. 2*nodes - 1
            // every helper wave converts the challenge for itself (no extra sync) -- if one of its lanes has a use for it
            Fr r = c;
            if (helper < N_HELPERS && (1 + helper < 2 * nodes || (a.weights_out && helper < n_w))) r = fr_to_mont_outlined(c);
            if (wave == OUT_WAVE) {
                // Outputs of this round, in Montgomery form as the reference holds them: the challenge, lo and hi, one conversion each on
                // three lanes side by side -- one product's worth of issue slots on the hash wave's SIMD, not three (with the rounds
                // shorter, three made this wave the last at the barrier).
                const uint32_t ol = threadIdx.x - 64 * OUT_WAVE;
                Fr m = ol == 1 ? told[2] : ol == 2 ? told[3] : c;
                if (ol < 3) m = fr_to_mont_outlined(m);
                if (absorb_sum) {
                    const Fr hi_m = shfl_fr(m, 2);
                    if (ol == 1) {
                        Fr sum_m = (a.first == 2) ? fr_from_arg(a.claimed) : (a.first == 3) ? load_fr(a.d_claimed, 0) : m + hi_m;
                        store_fr(st->sum, 0, sum_m);
                        if (a.host_delta) store_fr(st->sum + a.host_delta, 0, sum_m);
                    }
                }
                if (ol < 3) {
                    uint64_t* dst = ol == 0 ? challenges + 4 * (size_t)round : round_polys + 4 * (2 * (size_t)round + ol - 1);
                    store_fr(dst, 0, m);
                    if (a.host_delta) store_fr(dst + a.host_delta, 0, m);
                }
            }
            if (builder && depth >= 3) {
                // The tables the closing step of the NEXT round reads: digit multiples of D = new[q+2] - new[q], the new tree's level-2
                // difference.  With new[q] = old[q+4] + c (old[q+8] - old[q+4]) and new[q+2] = old[q+6] + c (old[q+10] - old[q+6]),
                //     D = X + c Y,  X = old[q+6] - old[q+4],  Y = (old[q+10] - old[q+8]) - X      (level 3 of the old tree),
                // so T_k = X 2^(28 k) + mont(c, to_mont(Y 2^(28 k))): one round of products for both parts side by side (the lanes of the
                // two half waves), one more for the part with c -- the canonical c: no conversion in front -- and the table is complete two
                // product latencies behind the barrier, half a round before the digest that it meets.
                const uint32_t q = 4 + b_v2;
                const Fr x = told[q + 6] - told[q + 4];
                const Fr y = (told[q + 10] - told[q + 8]) - x;
                const Fr p1 = (b_free ? x : y) * b_pow;
                Fr* slot = aff_stage + (bl & 31);
                if (b_free) *slot = p1;
                const Fr w = c * p1;                                              // (the first half's lanes' is the one that counts)
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");           // lanes read what other lanes of the wave wrote
                if (!b_free) affine_table_store(tbl_new + AFF_TABLE_WORDS * b_v2, b_k, *slot + w);
            }
            for (uint32_t q = 1 + helper; q < 2 * nodes && helper < N_HELPERS; q += N_HELPERS) {
                const uint32_t p = 1u << (31 - __builtin_clz(q));
                tnew[q] = told[q + p] + r * (told[q + 2 * p] - told[q + p]);
            }
            if (a.weights_out) {   // eq weights: the index gains the new variable as its least significant bit
                for (uint32_t b = helper; b < n_w && helper < N_HELPERS; b += N_HELPERS) {
                    Fr w1v = wold[b] * r;
                    wnew[2 * b + 1] = w1v;
                    wnew[2 * b] = wold[b] - w1v;
                }
            }
        }
        n_w <<= 1;
        --depth;
        ++round;
    }
    ZK_STAMP_AT(0, 40 + a.round0, 2);                   // rounds done
    // the output wave alone wrote to the mirror: its stores are out (system scope) before the barrier, the word follows behind it
    if (a.seq_word && wave == OUT_WAVE) __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
    __syncthreads();
    if (a.seq_word && threadIdx.x == 64 * OUT_WAVE) {
        __hip_atomic_store(a.seq_word, a.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        ZK_STAMP_AT(64 * OUT_WAVE, 40 + a.round0, 3);   // the proof is the host's
    }
    if (threadIdx.x == 0 && a.n_rounds) {   // what FiatShamirTranscript holds after a challenge(): fresh hasher + the digest
        Transcript tr;
        tr.init();
        tr.commit_words8(digest);
        tr.store(&st->transcript);
    }

    if (a.weights_out) {
        Fr* w = (a.n_rounds & 1) ? w1 : w0;
        for (uint32_t b = threadIdx.x; b < n_w; b += SMALL_BLOCK) store_fr(a.weights_out, b, w[b]);
    }
    if (a.final_out) {
        Fr* t = (a.n_rounds & 1) ? tree1 : tree0;
        const uint32_t cnt = 1u << depth;
        for (uint32_t j = threadIdx.x; j < cnt; j += SMALL_BLOCK) store_fr(a.final_out, j, t[cnt + j].to_mont());
    }
