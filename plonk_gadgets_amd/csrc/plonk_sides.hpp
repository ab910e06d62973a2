// plonk_sides.hpp -- the verifier's two sides from proof bytes: what verifier.sides computes on the host,
// one proof per lane, for a whole batch.  The per-proof routine is PG_HD over fr.hpp and g1_codec.hpp, so the kernels below and
// pg_plonk_sides_host (capi_sides.inc) run the same code.
//
//   decode      the proof's 11 commitments through g1_decode with the membership test: on the device a launch of its own, one lane
//               per commitment (11 x the lanes for what is 98 % of the instructions: about 1 820 Fq products a point against some
//               7 500 simple instructions a Keccak permutation), writing straight into the proof's rows 0..10 of `bases`.
//   transcript  Merlin over STROBE-128 over Keccak-f[1600], resumed from the key's seed (the state after the label, the circuit's
//               domain separator and the 15 key commitments).  The whole replay is ONE loop over a constant table of operations
//               (make_sides_program: 105 of them), so there is one byte step and one permutation in the code however many labels
//               and messages there are.  The sponge lives in memory the caller hands in -- LDS on the device, `S` words apart so
//               that the 64 lanes of a workgroup hit 64 banks -- because a seed's `pos` is a run-time value: the byte that is
//               absorbed next can be any of 166, and registers indexed at run time go to scratch.  Only the permutation holds the
//               state in registers (25 x 64 bits, every index static).
//   algebra     xi^n by log2 n squarings, PI(xi) as a running fraction, ONE inversion (of n (xi - 1) . n D . Z_H) for L1, PI and
//               t(xi), then the 23 x 2 coefficients.
//
// The table of a proof, 23 rows of (base, scalar a, scalar b); the check is e(sum a P, [tau]_2) e(sum b P, [1]_2) = 1:
//    0..10  the proof's a, b, c, d, z, t_1, t_2, t_3, t_4, w_z, w_zw                            (proof.COMMITMENTS)
//   11..21  the key's q_m, q_l, q_r, q_o, q_4, q_c, q_arith, left_sigma, right_sigma, out_sigma, fourth_sigma
//       22  the generator g of the opening key
// Equal points are not merged: a point in two rows carries two scalars, and the sum is the same.  A rejected proof's rows are
// identities and zeros -- its sums are the identity and its pairing product is 1, so the verdict is status == 0 AND check.
//
// With RANGE (pg_plonk_range_sides) the key record carries a twelfth point and the table a 24th row:
//       23  the key's q_range with (0, -v rho_range), rho_range = alpha^3 delta(b - 4a) + alpha^4 delta(c - 4b) + alpha^5 delta(a_w - 4c),
//           delta(f) = f (f-1)(f-2)(f-3): r(X)'s term of the range widget.  A record whose q_range is the identity
//           gets (identity, 0, 0), the sums it has without the row.  Rows 0..22 are the same either way.
#pragma once

#include "g1_codec.hpp"

namespace pg {

// per-proof status bytes (PG_SIDES_* of the C ABI); 1..4 are the PG_G1_* status of the first bad commitment
constexpr uint8_t kSidesOk = 0, kSidesBadEvaluation = 5, kSidesXiInDomain = 6, kSidesBadPublicInput = 7, kSidesBadKey = 8;
constexpr uint32_t kProofBytes = 1040, kSidesRows = 23, kSidesRangeRows = 24, kSidesCommitments = 11, kSidesEvaluations = 16, kSidesEvalOffset = 528;
constexpr uint32_t kSidesLanes = 64;  // lanes of a workgroup of plonk_sides_kernel
// words of sponge memory per proof: the STROBE state, the 64 bytes last squeezed, beta's 32 canonical bytes
constexpr uint32_t kSidesStateWords = 50, kSidesSqueezeAt = 50, kSidesBetaAt = 66, kSidesWords = 74;

// pg_plonk_key
struct PlonkKey {
    uint8_t state[200];
    uint8_t pos, pos_begin, cur_flags, log2_n;
    uint32_t reserved;
    Fr omega;
    G1A points[11];
    G1A g;
};
static_assert(sizeof(PlonkKey) == 1392, "pg_plonk_key is 1392 bytes");

// pg_plonk_range_key: a PlonkKey and the commitment of the range widget's selector
struct PlonkRangeKey {
    PlonkKey key;
    G1A q_range;
};
static_assert(sizeof(PlonkRangeKey) == 1488, "pg_plonk_range_key is 1488 bytes");

// the record and the rows of a proof, without and with the range widget's row
template <bool RANGE>
struct SidesTable {
    using Record = PlonkKey;
    static constexpr uint32_t kRows = kSidesRows;
};
template <>
struct SidesTable<true> {
    using Record = PlonkRangeKey;
    static constexpr uint32_t kRows = kSidesRangeRows;
};
PG_HD const PlonkKey *sides_key_of(const PlonkKey *rec) { return rec; }
PG_HD const PlonkKey *sides_key_of(const PlonkRangeKey *rec) { return &rec->key; }

// ---- Keccak-f[1600] -------------------------------------------------------------------------------------------------------------
PG_HD uint64_t rol64(uint64_t v, int s) { return s ? (v << s) | (v >> (64 - s)) : v; }

// lane (x, y) at a[x + 5 y]; the rounds stay a loop, everything inside a round is unrolled so that no index is a run-time value
PG_HD void keccak_f1600(uint64_t (&a)[25]) {
    const uint64_t RC[24] = {0x0000000000000001ull, 0x0000000000008082ull, 0x800000000000808aull, 0x8000000080008000ull,
                             0x000000000000808bull, 0x0000000080000001ull, 0x8000000080008081ull, 0x8000000000008009ull,
                             0x000000000000008aull, 0x0000000000000088ull, 0x0000000080008009ull, 0x000000008000000aull,
                             0x000000008000808bull, 0x800000000000008bull, 0x8000000000008089ull, 0x8000000000008003ull,
                             0x8000000000008002ull, 0x8000000000000080ull, 0x000000000000800aull, 0x800000008000000aull,
                             0x8000000080008081ull, 0x8000000000008080ull, 0x0000000080000001ull, 0x8000000080008008ull};
    constexpr int ROT[5][5] = {{0, 36, 3, 41, 18}, {1, 44, 10, 45, 2}, {62, 6, 43, 15, 61}, {28, 55, 25, 21, 56}, {27, 20, 39, 8, 14}};
#pragma unroll 1
    for (int r = 0; r < 24; r++) {
        uint64_t c[5], b[25];
#pragma unroll
        for (int x = 0; x < 5; x++) c[x] = a[x] ^ a[x + 5] ^ a[x + 10] ^ a[x + 15] ^ a[x + 20];
#pragma unroll
        for (int x = 0; x < 5; x++) {
            const uint64_t d = c[(x + 4) % 5] ^ rol64(c[(x + 1) % 5], 1);
#pragma unroll
            for (int y = 0; y < 5; y++) a[x + 5 * y] ^= d;
        }
#pragma unroll
        for (int x = 0; x < 5; x++) {
#pragma unroll
            for (int y = 0; y < 5; y++) b[y + 5 * ((2 * x + 3 * y) % 5)] = rol64(a[x + 5 * y], ROT[x][y]);
        }
#pragma unroll
        for (int y = 0; y < 5; y++) {
#pragma unroll
            for (int x = 0; x < 5; x++) a[x + 5 * y] = b[x + 5 * y] ^ (~b[(x + 1) % 5 + 5 * y] & b[(x + 2) % 5 + 5 * y]);
        }
        a[0] ^= RC[r];
    }
}

// ---- the transcript as a table ---------------------------------------------------------------------------------------------------
// An operation absorbs or squeezes `len` bytes; with STROBE flags it first begins a STROBE operation (two framing bytes, and a
// forced permutation for the flag C), without them it continues the one before (Merlin's length word: meta_ad(.., more)).
//   bits 0..3 kind, 4..11 flags, 12..19 len, 20..31 off
constexpr uint32_t kOpConst = 0,  // blob[off ..]: a label
    kOpProof = 1,                 // proof[off ..]: a commitment's 48 bytes or an evaluation's 32
    kOpLength = 2,                // the 4-byte little-endian length `off` (below 256)
    kOpBeta = 3,                  // beta's 32 canonical bytes, staged after the first challenge
    kOpSqueeze = 4;               // 64 bytes out: a challenge
constexpr uint32_t kStrobeI = 1, kStrobeA = 2, kStrobeC = 4, kStrobeM = 16, kStrobeR = 166;
constexpr uint32_t kSidesMaxOps = 112, kSidesBlobMax = 320, kSidesChallenges = 7;

struct SidesProgram {
    uint32_t ops[kSidesMaxOps];
    uint8_t blob[kSidesBlobMax];
    uint32_t phase_end[kSidesChallenges];  // ops[.. phase_end[k]) end with the squeeze of challenge k
    uint32_t n_ops, n_blob, n_phases;
};

constexpr uint32_t sides_op(uint32_t kind, uint32_t flags, uint32_t len, uint32_t off) { return kind | flags << 4 | len << 12 | off << 20; }

constexpr void sides_label(SidesProgram &p, const char *s) {
    uint32_t len = 0;
    while (s[len]) len++;
    p.ops[p.n_ops++] = sides_op(kOpConst, kStrobeM | kStrobeA, len, p.n_blob);
    for (uint32_t i = 0; i < len; i++) p.blob[p.n_blob++] = (uint8_t)s[i];
}
// Transcript.append_message(label, proof[off .. off + len))
constexpr void sides_append(SidesProgram &p, const char *label, uint32_t kind, uint32_t off, uint32_t len) {
    sides_label(p, label);
    p.ops[p.n_ops++] = sides_op(kOpLength, 0, 4, len);
    p.ops[p.n_ops++] = sides_op(kind, kStrobeA, len, off);
}
// Transcript.challenge_bytes(label, 64)
constexpr void sides_challenge(SidesProgram &p, const char *label) {
    sides_label(p, label);
    p.ops[p.n_ops++] = sides_op(kOpLength, 0, 4, 64);
    p.ops[p.n_ops++] = sides_op(kOpSqueeze, kStrobeI | kStrobeA | kStrobeC, 64, 0);
    p.phase_end[p.n_phases++] = p.n_ops;
}

// verifier.sides' transcript after the key's commitments, in its order; the challenges come out as
// beta, gamma, alpha, xi, v, v', u
constexpr SidesProgram make_sides_program() {
    SidesProgram p{};
    const char *wires[4] = {"w_l", "w_r", "w_o", "w_4"};
    for (uint32_t j = 0; j < 4; j++) sides_append(p, wires[j], kOpProof, 48 * j, 48);
    sides_challenge(p, "beta");
    sides_append(p, "beta", kOpBeta, 0, 32);
    sides_challenge(p, "gamma");
    sides_append(p, "z", kOpProof, 48 * 4, 48);
    sides_challenge(p, "alpha");
    const char *parts[4] = {"t_1", "t_2", "t_3", "t_4"};
    for (uint32_t j = 0; j < 4; j++) sides_append(p, parts[j], kOpProof, 48 * (5 + j), 48);
    sides_challenge(p, "z");
    const char *evals[16] = {"a_eval", "b_eval", "c_eval", "d_eval", "a_next_eval", "b_next_eval", "d_next_eval", "q_arith_eval",
                             "q_c_eval", "q_l_eval", "q_r_eval", "left_sigma_eval", "right_sigma_eval", "out_sigma_eval",
                             "lin_poly_eval", "perm_eval"};
    for (uint32_t j = 0; j < 16; j++) sides_append(p, evals[j], kOpProof, kSidesEvalOffset + 32 * j, 32);
    sides_challenge(p, "aggregate_witness");
    sides_append(p, "w_z", kOpProof, 48 * 9, 48);
    sides_challenge(p, "aggregate_witness");
    sides_append(p, "w_z_w", kOpProof, 48 * 10, 48);
    sides_challenge(p, "seperation challenge");  // (dusk's spelling)
    return p;
}
static_assert(make_sides_program().n_ops == 105 && make_sides_program().n_phases == kSidesChallenges &&
                  make_sides_program().n_blob <= kSidesBlobMax,
              "the table holds verifier.sides' 28 messages and 7 challenges");

// the evaluations' places in proof.EVALUATIONS
constexpr uint32_t kEvA = 0, kEvB = 1, kEvC = 2, kEvD = 3, kEvANext = 4, kEvBNext = 5, kEvDNext = 6, kEvQArith = 7, kEvQC = 8, kEvQL = 9,
                   kEvQR = 10, kEvLeftSigma = 11, kEvRightSigma = 12, kEvOutSigma = 13, kEvLin = 14, kEvPerm = 15;

PG_HD uint64_t sides_load_u64(const uint8_t *p) {
#if defined(__HIP_DEVICE_COMPILE__)
    return *reinterpret_cast<const uint64_t *>(p);  // (a device proof starts on 16 bytes and every field on 8)
#else
    uint64_t v = 0;
    for (int i = 7; i >= 0; i--) v = v << 8 | p[i];
    return v;
#endif
}

PG_HD Fr sides_raw_eval(const uint8_t *proof, uint32_t k) {
    const uint8_t *p = proof + kSidesEvalOffset + 32 * k;
    return Fr{{sides_load_u64(p), sides_load_u64(p + 8), sides_load_u64(p + 16), sides_load_u64(p + 24)}};
}
PG_HD Fr sides_eval(const uint8_t *proof, uint32_t k) { return fr_to_mont(sides_raw_eval(proof, k)); }

// BlsScalar::from_bytes_wide: lo + 2^256 hi mod r into Montgomery form, lo R^2 / R + hi R^3 / R (a factor below 2^256 and one
// below r leave a Montgomery product below 2 r, which its final subtraction reduces)
PG_HD Fr fr_from_wide(const Fr &lo, const Fr &hi) {
    const Fr r3{{0xc62c1807439b73afull, 0x1b3e0d188cf06990ull, 0x73d13c71c7b5f418ull, 0x6e2a5bb9c8db33e9ull}};  // R^3 mod r
    return fr_add(fr_mul(lo, fr_r2()), fr_mul(hi, r3));
}

// The replay: `mem` holds the seed's state in words 0..49 (word i at mem[i * S]); the seven challenges in Montgomery form.
template <int S>
PG_HD void sides_challenges(const uint8_t *proof, uint32_t *mem, uint32_t pos, uint32_t pos_begin, Fr (&ch)[kSidesChallenges]) {
    constexpr SidesProgram prog = make_sides_program();
    uint32_t pc = 0;
#pragma unroll 1
    for (uint32_t phase = 0; phase < kSidesChallenges; phase++) {
#pragma unroll 1
        for (; pc < prog.phase_end[phase]; pc++) {
            const uint32_t op = prog.ops[pc], kind = op & 15u, flags = (op >> 4) & 0xffu, len = (op >> 12) & 0xffu, off = op >> 20;
#pragma unroll 1
            for (int j = flags ? -2 : 0; j < (int)len; j++) {
                uint32_t b = 0;
                bool force = false;
                if (j == -2) {  // begin_op: the position the operation before began at, then the flags
                    b = pos_begin;
                    pos_begin = pos + 1;
                } else if (j == -1) {
                    b = flags;
                    force = (flags & kStrobeC) != 0;
                } else if (kind == kOpConst) {
                    b = prog.blob[off + j];
                } else if (kind == kOpProof) {
                    b = proof[off + j];
                } else if (kind == kOpLength) {
                    b = j == 0 ? off : 0u;
                } else if (kind == kOpBeta) {
                    b = (mem[(kSidesBetaAt + (j >> 2)) * S] >> (8 * (j & 3))) & 0xffu;
                }
                const uint32_t wi = pos >> 2, sh = 8 * (pos & 3u);
                uint32_t word = mem[wi * S];
                if (kind == kOpSqueeze && j >= 0) {  // the byte goes out and a zero takes its place
                    const uint32_t out = (word >> sh) & 0xffu, at = (kSidesSqueezeAt + (j >> 2)) * S;
                    word &= ~(0xffu << sh);
                    mem[at] = (j & 3) ? mem[at] | out << (8 * (j & 3)) : out;
                } else {
                    word ^= b << sh;
                }
                mem[wi * S] = word;
                pos++;
                if (pos == kStrobeR || (force && pos != 0)) {  // run_f
                    mem[(pos >> 2) * S] ^= pos_begin << (8 * (pos & 3u));
                    mem[((pos + 1) >> 2) * S] ^= 0x04u << (8 * ((pos + 1) & 3u));
                    mem[((kStrobeR + 1) >> 2) * S] ^= 0x80u << (8 * ((kStrobeR + 1) & 3u));
                    uint64_t a[25];
#pragma unroll
                    for (int i = 0; i < 25; i++) a[i] = (uint64_t)mem[(2 * i + 1) * S] << 32 | mem[2 * i * S];
                    keccak_f1600(a);
#pragma unroll
                    for (int i = 0; i < 25; i++) {
                        mem[2 * i * S] = (uint32_t)a[i];
                        mem[(2 * i + 1) * S] = (uint32_t)(a[i] >> 32);
                    }
                    pos = pos_begin = 0;
                }
            }
        }
        Fr lo, hi;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            lo.l[i] = (uint64_t)mem[(kSidesSqueezeAt + 2 * i + 1) * S] << 32 | mem[(kSidesSqueezeAt + 2 * i) * S];
            hi.l[i] = (uint64_t)mem[(kSidesSqueezeAt + 8 + 2 * i + 1) * S] << 32 | mem[(kSidesSqueezeAt + 8 + 2 * i) * S];
        }
        const Fr c = fr_from_wide(lo, hi);
#pragma unroll
        for (uint32_t k = 0; k < kSidesChallenges; k++)
            if (phase == k) ch[k] = c;
        if (phase == 0) {  // append_scalar(b"beta", beta) absorbs its canonical bytes
            const Fr raw = fr_from_mont(c);
#pragma unroll
            for (int i = 0; i < 4; i++) {
                mem[(kSidesBetaAt + 2 * i) * S] = (uint32_t)raw.l[i];
                mem[(kSidesBetaAt + 2 * i + 1) * S] = (uint32_t)(raw.l[i] >> 32);
            }
        }
    }
}

// omega^row, row < 2^m
PG_HD Fr sides_omega_pow(const Fr &omega, uint64_t row, uint32_t m) {
    Fr acc = fr_one(), base = omega;
#pragma unroll 1
    for (uint32_t bit = 0; bit < m; bit++) {
        if ((row >> bit) & 1) acc = fr_mul(acc, base);
        base = fr_square(base);
    }
    return acc;
}

// the range widget's delta(f) = f (f - 1)(f - 2)(f - 3), and 4 f
PG_HD Fr sides_delta(const Fr &f) {
    const Fr one = fr_one(), f1 = fr_sub(f, one), f2 = fr_sub(f1, one), f3 = fr_sub(f2, one);
    return fr_mul(fr_mul(f, f1), fr_mul(f2, f3));
}
PG_HD Fr sides_times4(const Fr &f) {
    const Fr f2 = fr_add(f, f);
    return fr_add(f2, f2);
}

// One proof.  cstat: the g1_decode status of its 11 commitments, whose points already stand in bases[0..10]; pi_rows / pi_vals
// [pi_begin, pi_end) its public inputs (Montgomery form); mem: kSidesWords words, S apart.  Writes the 23 bases, the 23 + 23
// scalars (24 with RANGE), *status and *where.  The tests are made in the order key, commitments, evaluations, public inputs, xi^n:
// the first that fails is the one reported.
template <int S, bool RANGE>
PG_HD void plonk_sides_one(const uint8_t *proof, const typename SidesTable<RANGE>::Record *keys, uint64_t n_keys, uint32_t key_index, const uint64_t *pi_rows,
                           const Fr *pi_vals, uint64_t pi_begin, uint64_t pi_end, const uint8_t *cstat, uint32_t *mem, G1A *bases,
                           Fr *sa, Fr *sb, uint8_t *status, uint8_t *where) {
    constexpr uint32_t kRows = SidesTable<RANGE>::kRows;
    uint8_t st = kSidesOk, wh = 0;
    const typename SidesTable<RANGE>::Record *rec = keys;
    const PlonkKey *key = sides_key_of(rec);
    uint32_t m = 0;
    if (key_index >= n_keys) {
        st = kSidesBadKey;
    } else {
        rec = keys + key_index;
        key = sides_key_of(rec);
        m = key->log2_n;
        if (m > 32 || key->pos >= kStrobeR || key->pos_begin > kStrobeR) st = kSidesBadKey;
    }
    if (st == kSidesOk) {
#pragma unroll 1
        for (uint32_t j = 0; j < kSidesCommitments; j++)
            if (st == kSidesOk && cstat[j] != kG1Ok) {
                st = cstat[j];
                wh = (uint8_t)j;
            }
    }
    if (st == kSidesOk) {
#pragma unroll 1
        for (uint32_t k = 0; k < kSidesEvaluations; k++)
            if (st == kSidesOk && !fr_raw_is_reduced(sides_raw_eval(proof, k))) {
                st = kSidesBadEvaluation;
                wh = (uint8_t)k;
            }
    }
    if (st == kSidesOk) {
#pragma unroll 1
        for (uint64_t k = pi_begin; k < pi_end; k++)
            if ((pi_rows[k] >> m) != 0 || !fr_raw_is_reduced(pi_vals[k])) st = kSidesBadPublicInput;  // (m <= 32: the shift is defined)
    }
    Fr ch[kSidesChallenges];
    Fr xin = fr_zero();
    if (st == kSidesOk) {
        const uint32_t *seed = reinterpret_cast<const uint32_t *>(key->state);
#pragma unroll 1
        for (uint32_t i = 0; i < kSidesStateWords; i++) mem[i * S] = seed[i];
        sides_challenges<S>(proof, mem, key->pos, key->pos_begin, ch);
        xin = ch[3];
#pragma unroll 1
        for (uint32_t i = 0; i < m; i++) xin = fr_square(xin);
        if (fr_eq(xin, fr_one())) st = kSidesXiInDomain;
    }
    *status = st;
    *where = wh;
    if (st != kSidesOk) {
#pragma unroll 1
        for (uint32_t row = 0; row < kRows; row++) {
            bases[row] = g1a_identity();
            sa[row] = fr_zero();
            sb[row] = fr_zero();
        }
        return;
    }
    const Fr beta = ch[0], gamma = ch[1], alpha = ch[2], xi = ch[3], v = ch[4], v2 = ch[5], u = ch[6];
    const Fr one = fr_one(), omega = key->omega;
    const Fr zh = fr_sub(xin, one);
    // PI(xi) = Z_H / n . N / D, N / D = sum_i v_i w^i / (xi - w^i) as a running fraction
    Fr pn = fr_zero(), pd = one;
#pragma unroll 1
    for (uint64_t k = pi_begin; k < pi_end; k++) {
        const Fr w = sides_omega_pow(omega, pi_rows[k], m);
        const Fr td = fr_sub(xi, w), tn = fr_mul(pi_vals[k], w);
        pn = fr_add(fr_mul(pn, td), fr_mul(tn, pd));
        pd = fr_mul(pd, td);
    }
    // one inversion for 1 / (n (xi - 1)), 1 / (n D) and 1 / Z_H; none of the three is zero once xi^n != 1
    const Fr nn = fr_from_u64(1ull << m);
    const Fr da = fr_mul(nn, fr_sub(xi, one)), db = fr_mul(nn, pd);
    const Fr dab = fr_mul(da, db);
    const Fr inv = fr_invert_or_zero(fr_mul(dab, zh));
    const Fr izh = fr_mul(inv, dab);
    const Fr inv_zh = fr_mul(inv, zh);  // 1 / (da db)
    const Fr l1 = fr_mul(zh, fr_mul(inv_zh, db));
    const Fr pi = fr_mul(fr_mul(zh, pn), fr_mul(inv_zh, da));

    const Fr a = sides_eval(proof, kEvA), b = sides_eval(proof, kEvB), c = sides_eval(proof, kEvC), d = sides_eval(proof, kEvD);
    const Fr zw = sides_eval(proof, kEvPerm), qa = sides_eval(proof, kEvQArith), lin = sides_eval(proof, kEvLin);
    Fr p3 = fr_add(fr_add(a, fr_mul(beta, sides_eval(proof, kEvLeftSigma))), gamma);
    p3 = fr_mul(p3, fr_add(fr_add(b, fr_mul(beta, sides_eval(proof, kEvRightSigma))), gamma));
    p3 = fr_mul(p3, fr_add(fr_add(c, fr_mul(beta, sides_eval(proof, kEvOutSigma))), gamma));
    const Fr a2l1 = fr_mul(fr_square(alpha), l1);
    const Fr ap3zw = fr_mul(fr_mul(alpha, p3), zw);
    const Fr n_xi = fr_sub(fr_sub(fr_add(lin, pi), fr_mul(ap3zw, fr_add(d, gamma))), a2l1);
    const Fr t_eval = fr_mul(n_xi, izh);
    // alpha prod_j (w_j + beta k_j xi + gamma), k = 1, 7, 13, 17
    const Fr bx = fr_mul(beta, xi);
    Fr zc = fr_mul(alpha, fr_add(fr_add(a, bx), gamma));
    zc = fr_mul(zc, fr_add(fr_add(b, fr_mul(bx, fr_from_u64(7))), gamma));
    zc = fr_mul(zc, fr_add(fr_add(c, fr_mul(bx, fr_from_u64(13))), gamma));
    zc = fr_mul(zc, fr_add(fr_add(d, fr_mul(bx, fr_from_u64(17))), gamma));

    // rows 11..22 are the key's
#pragma unroll 1
    for (uint32_t k = 0; k < 11; k++) bases[11 + k] = key->points[k];
    bases[22] = key->g;
#pragma unroll 1
    for (uint32_t row = 0; row < kRows; row++) sa[row] = fr_zero();
    sa[9] = one;
    sa[10] = u;

    // (the three sigma evaluations are read and converted a second time here rather than kept since P3: a product each, 24 registers)
    // F_xi: t(xi) and v r(xi), then v^2 .. v^12 over sigma_1..3, a, b, c, d, q_arith, q_c, q_l, q_r; u F_xiw: u v'^0..3 over
    // z, a, b, d.  The [1]_2 side carries -F and E g, E the same combination of the evaluations.
    const Fr uv1 = fr_mul(u, v2), uv2 = fr_mul(uv1, v2), uv3 = fr_mul(uv2, v2);
    const Fr vqa = fr_mul(v, qa);
    Fr value = fr_add(t_eval, fr_mul(v, lin));
    Fr vi = fr_mul(v, v);
    sb[18] = fr_neg(vi);
    value = fr_add(value, fr_mul(vi, sides_eval(proof, kEvLeftSigma)));
    vi = fr_mul(vi, v);
    sb[19] = fr_neg(vi);
    value = fr_add(value, fr_mul(vi, sides_eval(proof, kEvRightSigma)));
    vi = fr_mul(vi, v);
    sb[20] = fr_neg(vi);
    value = fr_add(value, fr_mul(vi, sides_eval(proof, kEvOutSigma)));
    vi = fr_mul(vi, v);
    sb[0] = fr_neg(fr_add(vi, uv1));
    value = fr_add(value, fr_mul(vi, a));
    vi = fr_mul(vi, v);
    sb[1] = fr_neg(fr_add(vi, uv2));
    value = fr_add(value, fr_mul(vi, b));
    vi = fr_mul(vi, v);
    sb[2] = fr_neg(vi);
    value = fr_add(value, fr_mul(vi, c));
    vi = fr_mul(vi, v);
    sb[3] = fr_neg(fr_add(vi, uv3));
    value = fr_add(value, fr_mul(vi, d));
    vi = fr_mul(vi, v);
    sb[17] = fr_neg(vi);
    value = fr_add(value, fr_mul(vi, qa));
    vi = fr_mul(vi, v);
    sb[16] = fr_neg(fr_add(vi, vqa));
    value = fr_add(value, fr_mul(vi, sides_eval(proof, kEvQC)));
    vi = fr_mul(vi, v);
    sb[12] = fr_neg(fr_add(vi, fr_mul(vqa, a)));
    value = fr_add(value, fr_mul(vi, sides_eval(proof, kEvQL)));
    vi = fr_mul(vi, v);
    sb[13] = fr_neg(fr_add(vi, fr_mul(vqa, b)));
    value = fr_add(value, fr_mul(vi, sides_eval(proof, kEvQR)));
    value = fr_add(value, fr_mul(u, zw));
    value = fr_add(value, fr_mul(uv1, sides_eval(proof, kEvANext)));
    value = fr_add(value, fr_mul(uv2, sides_eval(proof, kEvBNext)));
    value = fr_add(value, fr_mul(uv3, sides_eval(proof, kEvDNext)));
    sb[22] = value;
    sb[4] = fr_neg(fr_add(fr_mul(v, fr_add(zc, a2l1)), u));
    sb[5] = fr_neg_one();
    sb[6] = fr_neg(xin);
    const Fr xin2 = fr_square(xin);
    sb[7] = fr_neg(xin2);
    sb[8] = fr_neg(fr_mul(xin2, xin));
    sb[9] = fr_neg(xi);
    sb[10] = fr_neg(fr_mul(fr_mul(u, xi), omega));
    sb[11] = fr_neg(fr_mul(fr_mul(vqa, a), b));
    sb[14] = fr_neg(fr_mul(vqa, c));
    sb[15] = fr_neg(fr_mul(vqa, d));
    sb[21] = fr_mul(fr_mul(v, beta), ap3zw);
    if constexpr (RANGE) {
        // row 23, last: everything above is stored, and the four evaluations are read again rather than kept
        const G1A q = rec->q_range;
        bases[23] = q;
        Fr rho = fr_zero();
        if (!g1a_is_identity(q)) {
            const Fr ra = sides_eval(proof, kEvA), rb = sides_eval(proof, kEvB), rc = sides_eval(proof, kEvC);
            // alpha^3 (delta(b - 4a) + alpha (delta(c - 4b) + alpha delta(a_w - 4c)))
            rho = sides_delta(fr_sub(sides_eval(proof, kEvANext), sides_times4(rc)));
            rho = fr_add(fr_mul(rho, alpha), sides_delta(fr_sub(rc, sides_times4(rb))));
            rho = fr_add(fr_mul(rho, alpha), sides_delta(fr_sub(rb, sides_times4(ra))));
            rho = fr_mul(rho, fr_mul(fr_square(alpha), alpha));
        }
        sb[23] = fr_neg(fr_mul(v, rho));
    }
}

#if defined(__HIPCC__)
// One lane per commitment, commitment j of proof i at proofs + 1040 i + 48 j (16-byte aligned when proofs is): the point to
// bases[rows i + j], rows the table's rows per proof (23 or 24), the status to cstat[11 i + j].  Nothing waits on another lane.
__global__ __launch_bounds__(kThreads) void plonk_sides_decode_kernel(const uint8_t *proofs, uint64_t n, uint32_t rows, G1A *bases,
                                                                      uint8_t *cstat) {
    const uint64_t total = n * kSidesCommitments;
    for (uint64_t t = (uint64_t)blockIdx.x * kThreads + threadIdx.x; t < total; t += (uint64_t)gridDim.x * kThreads) {
        const uint64_t i = t / kSidesCommitments, j = t % kSidesCommitments;
        G1A p;
        const uint8_t st = g1_decode(g1_load_bytes(reinterpret_cast<const uint4 *>(proofs + i * kProofBytes + 48 * j), 0), true, &p);
        bases[i * rows + j] = p;
        cstat[t] = st;
    }
}

// One lane per proof, 64 lanes a workgroup; the sponge memory of lane l is the words lds[i * 64 + l].
template <bool RANGE>
__device__ __forceinline__ void plonk_sides_lane(const uint8_t *proofs, uint64_t n, const typename SidesTable<RANGE>::Record *keys,
                                                 uint64_t n_keys, const uint32_t *key_index, const uint64_t *pi_off, const uint64_t *pi_rows,
                                                 const Fr *pi_vals, const uint8_t *cstat, G1A *bases, Fr *scalars, uint64_t col_stride,
                                                 uint8_t *status, uint8_t *where) {
    constexpr uint32_t kRows = SidesTable<RANGE>::kRows;
    __shared__ uint32_t lds[kSidesWords * kSidesLanes];
    const uint64_t i = (uint64_t)blockIdx.x * kSidesLanes + threadIdx.x;
    if (i >= n) return;
    const uint64_t lo = pi_off ? pi_off[i] : 0, hi = pi_off ? pi_off[i + 1] : 0;
    plonk_sides_one<(int)kSidesLanes, RANGE>(proofs + i * kProofBytes, keys, n_keys, key_index ? key_index[i] : 0u, pi_rows, pi_vals, lo, hi,
                                             cstat + i * kSidesCommitments, lds + threadIdx.x, bases + i * kRows, scalars + i * kRows,
                                             scalars + col_stride + i * kRows, status + i, where + i);
}

__global__ __launch_bounds__(kSidesLanes) void plonk_sides_kernel(const uint8_t *proofs, uint64_t n, const PlonkKey *keys, uint64_t n_keys,
                                                                  const uint32_t *key_index, const uint64_t *pi_off, const uint64_t *pi_rows,
                                                                  const Fr *pi_vals, const uint8_t *cstat, G1A *bases, Fr *scalars,
                                                                  uint64_t col_stride, uint8_t *status, uint8_t *where) {
    plonk_sides_lane<false>(proofs, n, keys, n_keys, key_index, pi_off, pi_rows, pi_vals, cstat, bases, scalars, col_stride, status, where);
}

// ... with the range widget's row: records of 1488 bytes, 24 rows a proof
__global__ __launch_bounds__(kSidesLanes) void plonk_range_sides_kernel(const uint8_t *proofs, uint64_t n, const PlonkRangeKey *keys,
                                                                        uint64_t n_keys, const uint32_t *key_index, const uint64_t *pi_off,
                                                                        const uint64_t *pi_rows, const Fr *pi_vals, const uint8_t *cstat,
                                                                        G1A *bases, Fr *scalars, uint64_t col_stride, uint8_t *status,
                                                                        uint8_t *where) {
    plonk_sides_lane<true>(proofs, n, keys, n_keys, key_index, pi_off, pi_rows, pi_vals, cstat, bases, scalars, col_stride, status, where);
}
#endif

}  // namespace pg
