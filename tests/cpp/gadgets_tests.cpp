// tests/cpp/gadgets_tests.cpp -- the reference's own test-suite, re-expressed against the C++ host mirror
// (include/plonk_gadgets.hpp) of its public interface.
//
//   /root/reference/tests/range_gadgets_tests.rs    max_bound_test (:46-106), range_check_test (:108-201)
//   /root/reference/tests/scalar_gadgets_tests.rs   test_maybe_equal (:13-68), test_conditionally_select_0 (:70-122),
//                                                   test_conditionally_select_1 (:124-178), test_is_not_zero (:180-236)
//   /root/reference/src/range.rs:196-203            counting_scalar_bits
//   /root/reference/src/range.rs:205-233            scalar_decomposition_test
//
// Where the reference calls prover.prove()/verifier.verify() (dusk-plonk's proving system: out of scope here) this
// suite checks what that round trip establishes for the gadget layer:
//   * the prover-side circuit is satisfied on every row          (composer.check() == -1; "verify(...).is_ok()")
//   * a wrong outcome/witness leaves a row unsatisfied            ("verify(...).is_err()")
//   * the verifier-side circuit, built by the same closure from other witnesses, has the same selectors and wires
// and, beyond the reference, that every column equals the CPU oracle's composer limb for limb.
//
// Build + run: tests/test_gpu_cpp_host.py (g++; links libplonk_gadgets_hip.so, liboracle.so, libamdhip64.so).
#define __HIP_PLATFORM_AMD__ 1
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstring>
#include <functional>
#include <vector>

#include "plonk_gadgets.hpp"
extern "C" {
#include "gadgets.h"  // oracle (checker only)
}

using namespace plonk_gadgets;
using namespace plonk_gadgets::RangeGadgets;
using namespace plonk_gadgets::ScalarGadgets;

static int g_failed = 0, g_checks = 0;
#define CHECK(cond)                                                                  \
    do {                                                                             \
        g_checks++;                                                                  \
        if (!(cond)) { g_failed++; std::printf("  CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #cond); } \
    } while (0)

// ---- helpers ---------------------------------------------------------------------------------
struct Columns {
    std::vector<pg_scalar> q[5], vars;
    std::vector<uint64_t> w[3];
};

static Columns download(StandardComposer &c) {
    pg_columns d;
    pg_throw(pg_composer_columns(c.h, &d), "columns");
    pg_throw(pg_composer_sync(c.h), "sync");
    const size_t n = c.circuit_size(), nv = c.num_variables();
    Columns out;
    pg_scalar *qs[5] = {d.q_m, d.q_l, d.q_r, d.q_o, d.q_c};
    uint64_t *ws[3] = {d.w_l, d.w_r, d.w_o};
    for (int i = 0; i < 5; i++) { out.q[i].resize(n); (void)hipMemcpy(out.q[i].data(), qs[i], n * 32, hipMemcpyDeviceToHost); }
    for (int i = 0; i < 3; i++) { out.w[i].resize(n); (void)hipMemcpy(out.w[i].data(), ws[i], n * 8, hipMemcpyDeviceToHost); }
    out.vars.resize(nv);
    (void)hipMemcpy(out.vars.data(), d.var_values, nv * 32, hipMemcpyDeviceToHost);
    return out;
}

static bool same_structure(const Columns &a, const Columns &b) {
    for (int i = 0; i < 5; i++)
        if (a.q[i].size() != b.q[i].size() || std::memcmp(a.q[i].data(), b.q[i].data(), a.q[i].size() * 32)) return false;
    for (int i = 0; i < 3; i++)
        if (a.w[i] != b.w[i]) return false;
    return true;
}

static fr_t to_fr(const BlsScalar &s) { fr_t f; std::memcpy(f.l, s.s.l, 32); return f; }

// device composer == oracle composer, every limb of every live column
static bool equals_oracle(StandardComposer &dev, composer_t *ora) {
    const Columns c = download(dev);
    const size_t n = composer_circuit_size(ora), nv = composer_num_variables(ora);
    if (n != c.q[0].size() || nv != c.vars.size()) return false;
    const int sel[5] = {PG_Q_M, PG_Q_L, PG_Q_R, PG_Q_O, PG_Q_C};
    for (int i = 0; i < 5; i++)
        if (std::memcmp(composer_selector(ora, sel[i]), c.q[i].data(), n * 32)) return false;
    const int wi[3] = {PG_W_L, PG_W_R, PG_W_O};
    for (int i = 0; i < 3; i++)
        if (std::memcmp(composer_wire(ora, wi[i]), c.w[i].data(), n * 8)) return false;
    std::vector<fr_t> vals(nv);
    composer_values_dense(ora, vals.data());
    return std::memcmp(vals.data(), c.vars.data(), nv * 32) == 0;
}

static uint64_t g_rng = 0x9e3779b97f4a7c15ull;
static BlsScalar random_scalar() {  // BlsScalar::random(&mut rand::thread_rng())
    uint64_t raw[4];
    for (auto &x : raw) { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17; x = g_rng; }
    raw[3] %= 0x73eda753299d7d48ull;
    return BlsScalar::from_raw(raw);
}

// ---- tests/range_gadgets_tests.rs ----------------------------------------------------------------
static void max_bound_gadget(StandardComposer &composer, BlsScalar max_range, BlsScalar witness, bool result) {
    auto w = AllocatedScalar::allocate(composer, witness);
    auto [res, _n] = max_bound(composer, max_range, w);
    (void)_n;
    BlsScalar outcome = BlsScalar::zero();
    if (result) outcome = BlsScalar::one();
    composer.constrain_to_constant(res, outcome, std::nullopt);
}

static void range_check_gadget(StandardComposer &composer, BlsScalar max_range, BlsScalar min_range, BlsScalar witness,
                               bool result) {
    auto w = AllocatedScalar::allocate(composer, witness);
    auto res = range_check(composer, min_range, max_range, w);
    BlsScalar outcome = BlsScalar::zero();
    if (result) outcome = BlsScalar::one();
    composer.constrain_to_constant(res, outcome, std::nullopt);
}

static void max_bound_test(Engine &e) {
    struct TestCase { BlsScalar max_range, witness; bool expected_result; };
    const std::vector<TestCase> test_cases = {
        {BlsScalar::pow_of_2(128) - BlsScalar::one(), BlsScalar::pow_of_2(127), true},
        {BlsScalar::from(200), BlsScalar::from(100), true},
        {BlsScalar::from(100), BlsScalar::from(200), false},
        {BlsScalar::pow_of_2(128) - BlsScalar::one(), BlsScalar::pow_of_2(130), false},
    };
    for (const auto &tc : test_cases) {
        StandardComposer prover(e);  // Prover::default().mut_cs()
        max_bound_gadget(prover, tc.max_range, tc.witness, tc.expected_result);
        CHECK(prover.check() == -1);
        StandardComposer verifier(e);
        max_bound_gadget(verifier, tc.max_range, tc.witness, tc.expected_result);
        CHECK(same_structure(download(prover), download(verifier)));
        // the opposite outcome must not verify
        StandardComposer wrong(e);
        max_bound_gadget(wrong, tc.max_range, tc.witness, !tc.expected_result);
        CHECK(wrong.check() == (int64_t)wrong.circuit_size() - 1);
        // oracle, same calls
        composer_t *o = composer_new();
        uint64_t nb;
        var_t r = ::max_bound(o, to_fr(tc.max_range), allocated_scalar_allocate(o, to_fr(tc.witness)), &nb);
        composer_constrain_to_constant(o, r, tc.expected_result ? FR_ONE : FR_ZERO, nullptr);
        CHECK(equals_oracle(prover, o));
        composer_free(o);
    }
}

static void range_check_test(Engine &e) {
    struct TestCase { BlsScalar min_range, max_range, witness; bool expected_result; };
    const BlsScalar lo = BlsScalar::from(50000), hi = BlsScalar::from(250000);
    const std::vector<TestCase> test_cases = {
        {lo, hi, BlsScalar::from(50001), true},   {lo, hi, BlsScalar::from(250001), false},
        {lo, hi, BlsScalar::from(250000), false}, {lo, hi, BlsScalar::from(249000), true},
        {lo, hi, BlsScalar::from(50000), true},   {lo, hi, BlsScalar::from(49999), false},
        {BlsScalar::pow_of_2(126), BlsScalar::pow_of_2(127) + BlsScalar::one(), BlsScalar::pow_of_2(127) - BlsScalar::one(), true},
        {lo, hi, BlsScalar::from(18598), false},
    };
    for (const auto &tc : test_cases) {
        StandardComposer prover(e);
        range_check_gadget(prover, tc.max_range, tc.min_range, tc.witness, tc.expected_result);
        CHECK(prover.check() == -1);
        StandardComposer verifier(e);
        range_check_gadget(verifier, tc.max_range, tc.min_range, tc.witness, tc.expected_result);
        CHECK(same_structure(download(prover), download(verifier)));
        StandardComposer wrong(e);
        range_check_gadget(wrong, tc.max_range, tc.min_range, tc.witness, !tc.expected_result);
        CHECK(wrong.check() == (int64_t)wrong.circuit_size() - 1);
        composer_t *o = composer_new();
        var_t r = ::range_check(o, to_fr(tc.min_range), to_fr(tc.max_range), allocated_scalar_allocate(o, to_fr(tc.witness)));
        composer_constrain_to_constant(o, r, tc.expected_result ? FR_ONE : FR_ZERO, nullptr);
        CHECK(equals_oracle(prover, o));
        composer_free(o);
    }
}

// ---- tests/scalar_gadgets_tests.rs ------------------------------------------------------------------
static void test_maybe_equal(Engine &e) {
    auto is_equal_gadget = [](StandardComposer &composer, uint64_t num_1, uint64_t num_2, bool result) {
        auto a = AllocatedScalar::allocate(composer, BlsScalar::from(num_1));
        auto b = AllocatedScalar::allocate(composer, BlsScalar::from(num_2));
        auto bit = maybe_equal(composer, a, b);
        BlsScalar outcome = BlsScalar::zero();
        if (result) outcome = BlsScalar::one();
        composer.constrain_to_constant(bit, outcome, std::nullopt);
    };
    // Should pass as 100 == 100; the verifier builds the circuit from (0, 0)
    {
        StandardComposer prover(e), verifier(e);
        is_equal_gadget(prover, 100, 100, true);
        is_equal_gadget(verifier, 0, 0, true);
        CHECK(prover.check() == -1);
        CHECK(same_structure(download(prover), download(verifier)));
    }
    // 20 != 3330 -> bit = 0
    {
        StandardComposer prover(e), verifier(e), wrong(e);
        is_equal_gadget(prover, 20, 3330, false);
        is_equal_gadget(verifier, 0, 0, false);
        CHECK(prover.check() == -1);
        CHECK(same_structure(download(prover), download(verifier)));
        is_equal_gadget(wrong, 20, 3330, true);
        CHECK(wrong.check() >= 0);
        composer_t *o = composer_new();
        const allocated_scalar_t oa = allocated_scalar_allocate(o, fr_from_u64(20));  // sequenced: a before b
        const allocated_scalar_t ob = allocated_scalar_allocate(o, fr_from_u64(3330));
        var_t bit = ::maybe_equal(o, oa, ob);
        composer_constrain_to_constant(o, bit, FR_ZERO, nullptr);
        CHECK(equals_oracle(prover, o));
        composer_free(o);
    }
}

static void test_conditionally_select_0(Engine &e) {
    auto circuit = [](StandardComposer &composer, BlsScalar value, BlsScalar selector) {
        auto v = composer.add_input(value);
        auto s = composer.add_input(selector);
        auto res = conditionally_select_zero(composer, v, s);
        composer.constrain_to_constant(res, BlsScalar::zero(), std::nullopt);
    };
    // Selector set to 0 should select 0
    StandardComposer prover(e), verifier(e);
    circuit(prover, random_scalar(), BlsScalar::zero());
    circuit(verifier, random_scalar(), BlsScalar::zero());
    CHECK(prover.check() == -1);
    CHECK(same_structure(download(prover), download(verifier)));
    // Selector set to 1 shouldn't assign 0: constraining the result to 0 must fail
    StandardComposer prover2(e);
    circuit(prover2, random_scalar(), BlsScalar::one());
    CHECK(prover2.check() >= 0);
    CHECK(same_structure(download(prover2), download(verifier)));
    // ... and as the reference does it (tests/scalar_gadgets_tests.rs:108-119): prover.clear_witness(), the circuit again on
    // the SAME prover with the other witnesses -- same rows (found in place), other assignments, and it no longer verifies
    prover.clear_witness();
    CHECK(prover.circuit_size() == 3 && prover.num_variables() == 5);
    circuit(prover, random_scalar(), BlsScalar::one());
    CHECK(prover.check() >= 0);
    CHECK(same_structure(download(prover), download(verifier)));
    const auto st = prover.refresh_stats();
    CHECK(st.refreshing && st.rows_in_place == 2 && st.rows_rewritten == 0);  // the select's row and constrain_to_constant's
    prover.clear_witness();
    circuit(prover, random_scalar(), BlsScalar::zero());
    CHECK(prover.check() == -1);
}

static void test_conditionally_select_1(Engine &e) {
    auto circuit = [](StandardComposer &composer, BlsScalar value, BlsScalar selector, BlsScalar expected_result) {
        auto v = composer.add_input(value);
        auto s = composer.add_input(selector);
        auto res = conditionally_select_one(composer, v, s);
        composer.constrain_to_constant(res, BlsScalar::zero(), -expected_result);  // expected value as public input
    };
    // Selector set to 0 should assign 1
    StandardComposer prover(e);
    circuit(prover, random_scalar(), BlsScalar::zero(), BlsScalar::one());
    CHECK(prover.check() == -1);
    // Selector set to 1 should assign the randomly-generated value
    StandardComposer prover2(e);
    const BlsScalar rand = random_scalar();
    circuit(prover2, rand, BlsScalar::one(), rand);
    CHECK(prover2.check() == -1);
    CHECK(same_structure(download(prover), download(prover2)));  // public inputs are not part of the structure
    // tests/scalar_gadgets_tests.rs:168-177: clear_witness, then the second case on the first prover
    prover.clear_witness();
    circuit(prover, rand, BlsScalar::one(), rand);
    CHECK(prover.check() == -1);
    CHECK(same_structure(download(prover), download(prover2)));
    // a wrong public input does not verify
    StandardComposer wrong(e);
    circuit(wrong, rand, BlsScalar::one(), rand + BlsScalar::one());
    CHECK(wrong.check() == (int64_t)wrong.circuit_size() - 1);
    // oracle
    composer_t *o = composer_new();
    var_t v = composer_add_input(o, to_fr(rand)), s = composer_add_input(o, FR_ONE);
    var_t r = ::conditionally_select_one(o, v, s);
    fr_t pi = fr_neg(to_fr(rand));
    composer_constrain_to_constant(o, r, FR_ZERO, &pi);
    CHECK(equals_oracle(prover2, o));
    composer_free(o);
}

static void test_is_not_zero(Engine &e) {
    auto circuit = [](StandardComposer &composer, BlsScalar value, BlsScalar value_assigned) -> Result {
        auto v = composer.add_input(value);
        return is_non_zero(composer, v, value_assigned);
    };
    // Value & Value assigned set to 0 should err
    {
        StandardComposer prover(e);
        Result r = circuit(prover, BlsScalar::zero(), BlsScalar::zero());
        CHECK(r.is_err() && *r.err == Error::NonExistingInverse);
        // the partial emission of src/scalar.rs:69-71 is there: one input, one variable, one row
        CHECK(prover.circuit_size() == 3 + 1 && prover.num_variables() == 5 + 2);
    }
    // Value and value_assigned with different values should fail on verification
    {
        StandardComposer prover(e);
        CHECK(circuit(prover, random_scalar(), random_scalar()).is_ok());
        CHECK(prover.check() >= 0);
    }
    // Value & value assigned set correctly and != 0: this should pass
    {
        StandardComposer prover(e);
        const BlsScalar rand = random_scalar();
        CHECK(circuit(prover, rand, rand).is_ok());
        CHECK(prover.check() == -1);
        composer_t *o = composer_new();
        var_t v = composer_add_input(o, to_fr(rand));
        CHECK(::is_non_zero(o, v, to_fr(rand)) == GADGET_OK);
        CHECK(equals_oracle(prover, o));
        composer_free(o);
    }
}

// src/range.rs:196-203
static void counting_scalar_bits() {
    const BlsScalar zero = BlsScalar::zero(), one = BlsScalar::one(), three = BlsScalar::from(3);
    CHECK(pg_bits_count(&zero.s) == 1);
    CHECK(pg_bits_count(&one.s) == 1);
    CHECK(pg_bits_count(&three.s) == 2);
    const BlsScalar two_pow_128 = BlsScalar::pow_of_2(128);
    CHECK(pg_bits_count(&two_pow_128.s) == 129);
}

// src/range.rs:205-233
static void scalar_decomposition_test(Engine &e) {
    // Proving: -100 does not fit 8 bits, so is_eq = 0 and constraining it to zero holds
    StandardComposer prover(e);
    auto witness = AllocatedScalar::allocate(prover, -BlsScalar::from(100));
    auto [is_eq, bits] = scalar_decomposition_gadget(prover, 8, witness);
    prover.constrain_to_constant(is_eq, BlsScalar::zero(), std::nullopt);
    CHECK(bits.size() == 8);
    CHECK(prover.check() == -1);
    // Verification: the same circuit built from witness 1
    StandardComposer verifier(e);
    auto vw = AllocatedScalar::allocate(verifier, BlsScalar::from(1));
    auto [vis_eq, vbits] = scalar_decomposition_gadget(verifier, 8, vw);
    (void)vbits;
    verifier.constrain_to_constant(vis_eq, BlsScalar::zero(), std::nullopt);
    CHECK(same_structure(download(prover), download(verifier)));
    // oracle
    composer_t *o = composer_new();
    var_t r = ::scalar_decomposition_gadget(o, 8, allocated_scalar_allocate(o, fr_neg(fr_from_u64(100))), nullptr);
    composer_constrain_to_constant(o, r, FR_ZERO, nullptr);
    CHECK(equals_oracle(prover, o));
    composer_free(o);
}

// the reference panics where these throw: unknown Variable, composer overflow
static void panics_become_exceptions(Engine &e) {
    StandardComposer small(e, 8, 8);
    bool threw = false;
    try { range_check(small, BlsScalar::zero(), BlsScalar::pow_of_2(64), AllocatedScalar::allocate(small, BlsScalar::one())); }
    catch (const std::runtime_error &) { threw = true; }
    CHECK(threw);
    threw = false;
    try { small.boolean_gate(Variable{12345}); } catch (const std::runtime_error &) { threw = true; }
    CHECK(threw);
}

// ---- batched appends == the loops they stand for ------------------------------------------------------------
template <class T>
static T *to_device(const std::vector<T> &v) {
    T *d = nullptr;
    (void)hipMalloc(reinterpret_cast<void **>(&d), v.size() * sizeof(T) + 16);
    (void)hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
    return d;
}
static std::vector<uint64_t> sigma_of(StandardComposer &c, uint64_t padded) {
    uint64_t *d = nullptr;
    (void)hipMalloc(reinterpret_cast<void **>(&d), 4 * padded * 8);
    c.permutation(padded, d);
    pg_throw(pg_composer_sync(c.h), "sync");
    std::vector<uint64_t> h(4 * padded);
    (void)hipMemcpy(h.data(), d, h.size() * 8, hipMemcpyDeviceToHost);
    (void)hipFree(d);
    return h;
}

// One circuit built twice on the device: through the batched appends, and through loops of the reference-signature
// single calls.  Columns, Variables, satisfiability and the copy permutation must agree -- the first composer's sigma
// comes from the per-item linking, the second's from the sorted list, two different routes to the same cycles.
static void batched_appends_equal_loops(Engine &e) {
    const uint64_t batch = 45;
    std::vector<pg_scalar> wit, sel;
    for (uint64_t i = 0; i < batch; i++) {
        wit.push_back((i % 4 == 3 ? random_scalar() : BlsScalar::from(40000 + 7919 * i)).s);
        sel.push_back(BlsScalar::from(i & 1).s);
    }
    const BlsScalar mn = BlsScalar::from(50000), mx = BlsScalar::from(250000), bound = BlsScalar::pow_of_2(20);
    StandardComposer a(e, 1 << 17, 1 << 17), b(e, 1 << 17, 1 << 17);
    pg_scalar *d_wit = to_device(wit), *d_sel = to_device(sel);
    std::vector<uint64_t> zeros(batch, 0);
    uint64_t *d_res = to_device(zeros), *d_res2 = to_device(zeros);

    // batched
    Batched::range_check(a, mn, mx, d_wit, batch, d_res);
    const Variable fw = Batched::allocate(a, d_wit, batch), fs = Batched::allocate(a, d_sel, batch);
    std::vector<uint64_t> wv, sv;
    for (uint64_t i = 0; i < batch; i++) { wv.push_back(fw.index + i); sv.push_back(fs.index + i); }
    uint64_t *d_wv = to_device(wv), *d_sv = to_device(sv);
    const uint64_t nb = Batched::max_bound_allocated(a, bound, d_wv, d_wit, batch, d_res2);
    Batched::conditionally_select_one(a, d_wv, d_sv, batch, nullptr);
    Batched::maybe_equal(a, d_res, d_res2, batch, nullptr);
    Batched::constrain_to_constant(a, d_res2, BlsScalar::one(), batch);
    Batched::boolean_gate(a, d_res, batch);
    uint64_t errs = 0;
    CHECK(Batched::is_non_zero(a, d_wv, batch, nullptr, &errs).is_ok() && errs == 0);
    CHECK(Batched::is_non_zero(a, d_sv, batch, nullptr, &errs).is_err() && errs == (batch + 1) / 2);

    // the loops
    std::vector<Variable> r1, r2;
    for (uint64_t i = 0; i < batch; i++)
        r1.push_back(range_check(b, mn, mx, AllocatedScalar::allocate(b, BlsScalar(wit[i]))));
    std::vector<AllocatedScalar> aw, as;
    for (uint64_t i = 0; i < batch; i++) aw.push_back(AllocatedScalar::allocate(b, BlsScalar(wit[i])));
    for (uint64_t i = 0; i < batch; i++) as.push_back(AllocatedScalar::allocate(b, BlsScalar(sel[i])));
    CHECK(aw[0].var == fw && as[0].var == fs);
    uint64_t nb2 = 0;
    for (uint64_t i = 0; i < batch; i++) {
        auto [v, n] = max_bound(b, bound, aw[i]);
        r2.push_back(v);
        nb2 = n;
    }
    CHECK(nb == nb2);
    for (uint64_t i = 0; i < batch; i++) conditionally_select_one(b, aw[i].var, as[i].var);
    for (uint64_t i = 0; i < batch; i++)
        maybe_equal(b, AllocatedScalar{r1[i], b.value(r1[i])}, AllocatedScalar{r2[i], b.value(r2[i])});
    for (uint64_t i = 0; i < batch; i++) b.constrain_to_constant(r2[i], BlsScalar::one(), std::nullopt);
    for (uint64_t i = 0; i < batch; i++) b.boolean_gate(r1[i]);
    for (uint64_t i = 0; i < batch; i++) CHECK(is_non_zero(b, aw[i].var, aw[i].scalar).is_ok());
    uint64_t loop_errs = 0;
    for (uint64_t i = 0; i < batch; i++) loop_errs += is_non_zero(b, as[i].var, as[i].scalar).is_err();
    CHECK(loop_errs == errs);

    std::vector<uint64_t> res(batch);
    (void)hipMemcpy(res.data(), d_res, batch * 8, hipMemcpyDeviceToHost);
    for (uint64_t i = 0; i < batch; i++) CHECK(res[i] == r1[i].index);
    CHECK(a.circuit_size() == b.circuit_size() && a.num_variables() == b.num_variables());
    const Columns ca = download(a), cb = download(b);
    CHECK(same_structure(ca, cb));
    CHECK(ca.vars.size() == cb.vars.size() && std::memcmp(ca.vars.data(), cb.vars.data(), ca.vars.size() * 32) == 0);
    CHECK(a.check() == b.check());
    uint64_t padded = 1;
    while (padded < a.circuit_size()) padded <<= 1;
    CHECK(sigma_of(a, padded) == sigma_of(b, padded));
    for (void *p : {(void *)d_wit, (void *)d_sel, (void *)d_res, (void *)d_res2, (void *)d_wv, (void *)d_sv}) (void)hipFree(p);
}

// The Batched:: wrappers of the widgets, the comparison, the weighted sum and the ragged ladders (include/plonk_gadgets.hpp) against
// the C ABI they forward to: every call through the C++ mirror on one composer and through pg_composer_* on a second.  Every argument
// of a call differs from its neighbours (x from y, min from max, coefficients from constants, num_bits from the batch), so a wrapper
// that swaps two of them builds another circuit -- or is refused, which is counted as a failure too.
static void wrappers_equal_the_c_abi(Engine &e) {
    const uint64_t batch = 8, terms = 8, segments = 3;
    std::vector<pg_scalar> wit, mins, maxs, rmin, rmax, bounds, coeff, constant;
    for (uint64_t i = 0; i < batch; i++) {
        wit.push_back(BlsScalar::from(3 + i).s);        // below 2^4, and inside every interval below
        mins.push_back(BlsScalar::from(1 + i % 3).s);
        maxs.push_back(BlsScalar::from(16 + i % 3).s);  // max - min = 15 < 2^4
        rmin.push_back(BlsScalar::from(i).s);
        rmax.push_back(BlsScalar::from(100 + 9 * i).s);
        bounds.push_back(BlsScalar::from(50 + 11 * i).s);
        coeff.push_back(BlsScalar::from(2 + i).s);
    }
    for (uint64_t s = 0; s < terms; s++) constant.push_back(BlsScalar::from(1000 + s).s);  // (as long as coeff: a swap stays inside both)
    const std::vector<uint64_t> seg_off = {0, 2, 5, 8}, zeros(batch, 0);
    pg_scalar *d_wit = to_device(wit), *d_min = to_device(mins), *d_max = to_device(maxs), *d_rmin = to_device(rmin),
              *d_rmax = to_device(rmax), *d_bounds = to_device(bounds), *d_coeff = to_device(coeff), *d_constant = to_device(constant);
    uint64_t *d_off = to_device(seg_off);
    const BlsScalar lo = BlsScalar::from(2), hi = BlsScalar::from(17);
    StandardComposer a(e, 1 << 14, 1 << 14), b(e, 1 << 14, 1 << 14);
    std::vector<std::vector<uint64_t>> ra, rb;  // the result Variables, call by call
    uint64_t *d_res = to_device(zeros);
    uint32_t *d_nb = to_device(std::vector<uint32_t>(batch, 0));
    auto results = [&](std::vector<std::vector<uint64_t>> &into, StandardComposer &c, uint64_t count) {
        pg_throw(pg_composer_sync(c.h), "sync");
        std::vector<uint64_t> r(count);
        (void)hipMemcpy(r.data(), d_res, count * 8, hipMemcpyDeviceToHost);
        into.push_back(r);
    };
    try {
        for (StandardComposer *c : {&a, &b}) {
            const bool cpp = c == &a;
            const Variable first = Batched::allocate(*c, d_wit, batch);
            std::vector<uint64_t> x, y;
            for (uint64_t i = 0; i < batch; i++) { x.push_back(first.index + i); y.push_back(first.index + (i + 3) % batch); }
            uint64_t *d_x = to_device(x), *d_y = to_device(y);
            if (cpp) {
                Batched::range_gate(*c, d_x, 4, batch - 2);
                Batched::interval_gate(*c, d_x, lo.s, hi.s, 6, batch - 1);
                Batched::interval_gate(*c, d_x, d_min, d_max, 4, batch);
                Batched::is_less_equal(*c, d_x, d_y, 4, false, batch - 3, d_res);
                results(ra, *c, batch - 3);
                Batched::is_less_equal(*c, d_x, d_y, 6, true, batch, d_res);
                results(ra, *c, batch);
                Batched::weighted_sum(*c, d_x, d_off, d_coeff, d_constant, terms, segments, d_res);
                results(ra, *c, segments);
                Batched::range_check_ragged(*c, d_rmin, d_rmax, d_wit, batch, d_res, d_nb);
                results(ra, *c, batch);
                Batched::max_bound_ragged(*c, d_bounds, d_wit, batch, d_res, d_nb);
                results(ra, *c, batch);
            } else {
                pg_throw(pg_composer_range_gate_batch(c->h, d_x, 4, batch - 2), "range_gate");
                pg_throw(pg_composer_interval_gate_batch(c->h, d_x, &lo.s, &hi.s, 6, batch - 1), "interval_gate");
                pg_throw(pg_composer_interval_gate_ragged_batch(c->h, d_x, d_min, d_max, 4, batch), "interval_gate (ragged)");
                pg_throw(pg_composer_is_less_equal_batch(c->h, d_x, d_y, 4, 0, batch - 3, d_res), "is_less_equal");
                results(rb, *c, batch - 3);
                pg_throw(pg_composer_is_less_equal_batch(c->h, d_x, d_y, 6, 1, batch, d_res), "is_less_equal (strict)");
                results(rb, *c, batch);
                pg_throw(pg_composer_weighted_sum_ragged_batch(c->h, d_x, d_off, d_coeff, d_constant, terms, segments, d_res), "weighted_sum");
                results(rb, *c, segments);
                pg_throw(pg_composer_range_check_ragged_batch(c->h, d_rmin, d_rmax, d_wit, batch, d_res, d_nb), "range_check_ragged");
                results(rb, *c, batch);
                pg_throw(pg_composer_max_bound_ragged_batch(c->h, d_bounds, d_wit, batch, d_res, d_nb), "max_bound_ragged");
                results(rb, *c, batch);
            }
            pg_throw(pg_composer_sync(c->h), "sync");
            (void)hipFree(d_x);
            (void)hipFree(d_y);
        }
        CHECK(a.circuit_size() == b.circuit_size() && a.num_variables() == b.num_variables() && a.circuit_size() > 3);
        const Columns ca = download(a), cb = download(b);
        CHECK(same_structure(ca, cb));
        CHECK(ca.vars.size() == cb.vars.size() && std::memcmp(ca.vars.data(), cb.vars.data(), ca.vars.size() * 32) == 0);
        CHECK(a.check() == -1 && b.check() == -1);
        CHECK(ra == rb && ra.size() == 5);
    } catch (const std::exception &ex) {
        std::printf("  a call was refused: %s\n", ex.what());
        CHECK(false);
    }
    for (void *p : {(void *)d_wit, (void *)d_min, (void *)d_max, (void *)d_rmin, (void *)d_rmax, (void *)d_bounds, (void *)d_coeff,
                    (void *)d_constant, (void *)d_off, (void *)d_res, (void *)d_nb})
        (void)hipFree(p);
}

// BlsScalar::invert as the gadgets use it (src/scalar.rs:73,121): x * x^-1 == 1, zero has none
static void scalar_invert() {
    BlsScalar inv;
    for (uint64_t v : {1ull, 2ull, 7ull, 1ull << 30, (1ull << 60) + 1, ~0ull}) {
        CHECK(BlsScalar::from(v).invert(&inv));
        CHECK(BlsScalar::from(v) * inv == BlsScalar::one());
    }
    CHECK((-BlsScalar::one()).invert(&inv) && inv == -BlsScalar::one());
    CHECK(!BlsScalar::zero().invert(&inv) && inv == BlsScalar::zero());
}

// the reference's loop, one call at a time (tests/range_gadgets_tests.rs:29-44): recorded and flushed as few launches, the
// same columns as with recording off and as the oracle's loop
static void single_calls_are_queued(Engine &e) {
    const BlsScalar mn = BlsScalar::from(1000), mx = BlsScalar::from(90000);
    composer_t *ora = composer_new();
    StandardComposer queued(e, 1 << 17, 1 << 18), direct(e, 1 << 17, 1 << 18);
    direct.queue(false);
    const auto q0 = queued.queue_stats();
    for (uint64_t i = 0; i < 100; i++) {
        const BlsScalar w = BlsScalar::from(500 + 997 * i);
        const var_t ov = ::range_check(ora, to_fr(mn), to_fr(mx), allocated_scalar_allocate(ora, to_fr(w)));
        const Variable a = range_check(queued, mn, mx, AllocatedScalar::allocate(queued, w));
        const Variable b = range_check(direct, mn, mx, AllocatedScalar::allocate(direct, w));
        CHECK(a.index == ov && b.index == ov);
    }
    CHECK(queued.queue_stats().pending >= 200);  // nothing has reached the device yet
    queued.flush();
    const auto q1 = queued.queue_stats();
    CHECK(q1.pending == 0 && q1.flushes == q0.flushes + 1 && q1.launches <= q0.launches + 2);
    CHECK(equals_oracle(queued, ora) && equals_oracle(direct, ora));
    CHECK(queued.check() == -1 && direct.check() == -1);
    composer_free(ora);
}

int main() {
    Engine e(0);
    struct { const char *name; std::function<void()> fn; } tests[] = {
        {"counting_scalar_bits", [&] { counting_scalar_bits(); }},
        {"scalar_invert", [&] { scalar_invert(); }},
        {"batched_appends_equal_loops", [&] { batched_appends_equal_loops(e); }},
        {"single_calls_are_queued", [&] { single_calls_are_queued(e); }},
        {"wrappers_equal_the_c_abi", [&] { wrappers_equal_the_c_abi(e); }},
        {"scalar_decomposition_test", [&] { scalar_decomposition_test(e); }},
        {"max_bound_test", [&] { max_bound_test(e); }},
        {"range_check_test", [&] { range_check_test(e); }},
        {"test_maybe_equal", [&] { test_maybe_equal(e); }},
        {"test_conditionally_select_0", [&] { test_conditionally_select_0(e); }},
        {"test_conditionally_select_1", [&] { test_conditionally_select_1(e); }},
        {"test_is_not_zero", [&] { test_is_not_zero(e); }},
        {"panics_become_exceptions", [&] { panics_become_exceptions(e); }},
    };
    for (auto &t : tests) {
        const int before = g_failed;
        t.fn();
        std::printf("test %s ... %s\n", t.name, g_failed == before ? "ok" : "FAILED");
    }
    std::printf("%d checks, %d failed\n", g_checks, g_failed);
    return g_failed ? 1 : 0;
}
