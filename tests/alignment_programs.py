"""TEST INFRASTRUCTURE: the programs of the alignment sweep (tests/test_gpu_append_alignment.py, DESIGN section 5 "Alignments"), one
per kind of append, made call for call on the device composer and on the C oracle's through Both; dev = None runs the oracle alone
(tests/test_append_alignment_programs.py: every program is satisfiable and fits its fixed capacity with the room the two rules ask).

An append's writers derive their store pattern from the address of the call's first row and first Variable: 16 row alignments
((first row) mod 16: the 128-byte line of a wire column, the 8-byte parity of its pairs among them; a selector line is 4 rows) and 4
Variable alignments ((first Variable) mod 4).  A program visits all 64 targets; at each it allocates what the call refers to, pads
to the target -- boolean_gate(zero_var) for rows, add_input_batch for Variables, both residues asserted, not assumed -- and makes the
call with batches 1, 2 and 3 of each of the kind's shapes (a shape with an odd and one with an even number of rows per item, where
the kind has both).  Then one batch of the kind's tile width + 1 at each of the 16 row residues (Variable residue = row residue mod
4): the call crosses a tile boundary at every row alignment.  For the uniform kinds W rows-per-item is a multiple of 16 and W
Variables-per-item a multiple of 4, so their second tile starts at the first one's residues; the ragged kinds and the weighted sum
(segments of 2 and 3 terms) get another alignment there.

Everything PUBLIC in a program (Variables referred to, bounds, coefficients, where an item fails) is fixed; the witness scalars come
from wit_seed, so the same program on another seed is the same circuit on other assignments (the values-only refresh).

A new emitter joins the sweep with one Kind in KINDS: prepare() allocates the Variables the call refers to and draws its witnesses,
call() makes it through a Both method, `tile` is its tile width + 1, CAPACITY its composer's fixed size."""
import ctypes as C
import random

from tests import capacity_views as cv
from tests import weighted_sum_oracle as wso
from tests.compare_programs import CompareBoth
from tests.widget_programs import R

# tile widths, from the headers: PG_RC_W = 32 (csrc/range_gadgets.hpp: RangeCheckGD and RangeBoundsGD), PG_MB_W = 16 (MaxBoundGD),
# DecompositionGD::W = 32; W = 256 for the widgets (csrc/range_gate.hpp, interval_gate.hpp, compare_gate.hpp) and the small items
# (csrc/scalar_gadgets.hpp).  The gadgets on Variables from elsewhere take 33: two tiles of 16 or one of 32, and one item more.
RC_TILE, MB_TILE, DEC_TILE, SMALL_TILE = 32 + 1, 16 + 1, 32 + 1, 256 + 1
BATCHES = (1, 2, 3)


class AllBoth(CompareBoth, wso.Both):
    """every call of the three replay classes on one pair of composers (wid: CompareWidgets, which has the other widgets too)"""


def weighted_sum_tile():
    """T + 1 terms: one more than weighted_sum_write_kernel's tile (pg_weighted_sum_geometry)"""
    from plonk_gadgets_amd import _lib
    t, p = C.c_uint32(), C.c_uint32()
    assert _lib.load().pg_weighted_sum_geometry(C.byref(t), C.byref(p)) == 0
    return int(t.value) + 1


class Kind:
    def __init__(self, name, shapes, tile, prepare, call, refreshed=True):
        self.name, self.shapes, self._tile, self.prepare, self.call, self.refreshed = name, shapes, tile, prepare, call, refreshed

    @property
    def tile(self):
        return self._tile() if callable(self._tile) else self._tile

    def __repr__(self):
        return self.name


def _inputs(both, values):
    return both.add_input_batch([v % R for v in values])


def _scalars(w, k, nonzero=False):
    return [w.randrange(1 if nonzero else 0, R) for _ in range(k)]


def _alternate(pair, k, shape):
    return [pair[(i + shape) % 2] for i in range(k)]


# ---- the widgets on existing Variables (emit_kernel) ---------------------------------------------------------------------------
RANGE_BITS = (4, 8)        # 2 rows and 1 Variable an item; 3 rows and 3 Variables
INTERVAL_BITS = (2, 8)     # always an even number of rows
COMPARE_BITS = (2, 6)      # 2 rows and 2 Variables; 3 rows and 4 Variables
LADDER_BOUNDS = (2, 3)     # ladder items of fewer than 16 rows (and 19: range_check on 3)


def _range_gate(shape):
    bits = RANGE_BITS[shape]
    return (lambda both, w, k: _inputs(both, [w.randrange(1 << bits) for _ in range(k)]),
            lambda both, vs: both.range_gate_batch(vs, bits))


def _interval(shape, ragged):
    bits = INTERVAL_BITS[shape]
    top = (1 << bits) - 1

    def los(k):
        return [5 + 3 * (i % 4) for i in range(k)] if ragged else [5] * k

    def prepare(both, w, k):
        return _inputs(both, [lo + w.randrange(top + 1) for lo in los(k)])

    def call(both, vs):
        lo = los(len(vs))
        if ragged:
            both.interval_gate_ragged_batch(vs, lo, [x + top for x in lo], bits)
        else:
            both.interval_gate_batch(vs, lo[0], lo[0] + top, bits)
    return prepare, call


def _compare(shape, strict):
    bits = COMPARE_BITS[shape]

    def prepare(both, w, k):
        vs = _inputs(both, [w.randrange(1 << bits) for _ in range(2 * k)])
        return vs[:k], vs[k:]
    return prepare, lambda both, xy: both.is_less_equal_each(xy[0], xy[1], bits, strict)


def _weighted_sum(shape):
    """batch = segments of 2 and 3 terms in turn (shape 0 begins with 2 and has coeffs and constants, shape 1 begins with 3 and has
    neither); the tile run has T + 1 TERMS in such segments"""
    def sizes(k):
        if k in BATCHES:
            return _alternate((2, 3), k, shape)
        out, left = [], k
        while left:
            s = (2, 3)[(len(out) + shape) % 2]
            s = left if left - s < 2 else s
            out.append(s)
            left -= s
        return out

    def prepare(both, w, k):
        return k, _inputs(both, _scalars(w, sum(sizes(k))))

    def call(both, ctx):
        k, vs = ctx
        off = [0]
        for s in sizes(k):
            off.append(off[-1] + s)
        pub = random.Random(7 * len(vs) + shape)
        coeffs = [pub.choice([0, 1, R - 1, pub.randrange(R)]) for _ in vs] if shape == 0 else None
        constants = [pub.choice([0, R - 1, pub.randrange(R)]) for _ in off[1:]] if shape == 0 else None
        both.weighted_sum_ragged_batch(vs, off, coeffs, constants)
    return prepare, call


# ---- ladders ---------------------------------------------------------------------------------------------------------------------
def _ladder(method, shape, ragged=False, allocated=False, bounds=LADDER_BOUNDS):
    def prepare(both, w, k):
        values = [w.randrange(2 * b + 1) for b in (_alternate(bounds, k, shape) if ragged else [bounds[shape]] * k)]
        return _inputs(both, values) if allocated else values

    def call(both, x):
        b, rag = bounds[shape], _alternate(bounds, len(x), shape)
        {"range_check_batch": lambda: both.range_check_batch(0, b, x),
         "max_bound_batch": lambda: both.max_bound_batch(b, x),
         "max_bound_ragged_batch": lambda: both.max_bound_ragged_batch(rag, x),
         "range_check_ragged_batch": lambda: both.range_check_ragged_batch([0] * len(x), rag, x),
         "range_check_allocated_batch": lambda: both.range_check_allocated_batch(0, b, x),
         "max_bound_allocated_batch": lambda: both.max_bound_allocated_batch(b, x),
         "scalar_decomposition_batch": lambda: both.scalar_decomposition_batch(b, x)}[method]()
    return prepare, call


# ---- small items and gate batches ---------------------------------------------------------------------------------------------
# is_non_zero_batch and scalar_mix_batch are swept twice.  Without a failing item they are found in place by the values-only refresh at all 64
# targets (the inversion pre-pass writes z in place there too).  In the `_failing` kinds this item of every batch of 3 or more has v = 0 and
# stops at its error: the early-stop path at the swept alignments; such a batch is never found in place and ends the refresh.
FAILING_ITEM = 1


def _two_inputs(method, second):
    """second: what the second array's Variables hold -- "bit", "any", or "equal" (every other one the first array's value)"""
    def prepare(both, w, k):
        a = _scalars(w, k)
        b = {"bit": [w.randrange(2) for _ in range(k)], "any": _scalars(w, k),
             "equal": [x if i % 2 == 0 else y for i, (x, y) in enumerate(zip(a, _scalars(w, k)))]}[second]
        vs = _inputs(both, a + b)
        return vs[:k], vs[k:]
    return prepare, lambda both, ab: getattr(both, method)(ab[0], ab[1])


def _is_non_zero(failing):
    def prepare(both, w, k):
        return _inputs(both, [0 if failing and i == FAILING_ITEM and k >= 3 else v for i, v in enumerate(_scalars(w, k, nonzero=True))])
    return prepare, lambda both, vs: both.is_non_zero_batch(vs)


def _scalar_mix(failing):
    def prepare(both, w, k):
        v = [0 if failing and i == FAILING_ITEM and k >= 3 else x for i, x in enumerate(_scalars(w, k, nonzero=True))]
        return [v] + [[w.choice([0, 1, w.randrange(R)]) for _ in range(k)] for _ in range(4)]
    return prepare, lambda both, x: both.scalar_mix_batch(*x)


def _gates(method):
    def prepare(both, w, k):
        if method == "boolean_gate_batch":
            return _inputs(both, [w.randrange(2) for _ in range(k)])
        if method == "constrain_to_constant_batch":
            return _inputs(both, [12345] * k)       # (a public constant: these inputs are the same on every witness seed)
        if method == "add_input_batch":
            return _scalars(w, k)
        vs = _inputs(both, _scalars(w, 2 * k))
        return vs[:k], vs[k:]

    def call(both, x):
        {"add_batch": lambda: both.add_batch(3, x[0], 5, x[1], 1),
         "mul_batch": lambda: both.mul_batch(2, x[0], x[1], 7),
         "poly_gate_batch": lambda: both.poly_gate_batch(x[0], x[0], x[1], [0, 9, R - 9, 0, 0]),     # 9 a - 9 a = 0 whatever a holds
         "boolean_gate_batch": lambda: both.boolean_gate_batch(x),
         "constrain_to_constant_batch": lambda: both.constrain_to_constant_batch(x, 12345),
         "add_input_batch": lambda: both.add_input_batch(x)}[method]()
    return prepare, call


# ---- runs of single calls, flushed by the queue as one launch with its items stride_rows apart -------------------------------
# flush_loop (csrc/capi_composer.inc) takes a run for ONE strided launch when it holds at least two bodies, each an allocate + gadget pair
# FOLLOWED by a gate that creates no Variable.  So every call of a batch of 2 or more is followed by such a gate: batches 2, 3 and QUEUE_RUN
# reach EmitOut::stride_rows with 2, 3 and 5 items (an even and two odd counts); a batch of 1 is a single call, flushed alone, without a
# gate behind it -- the odd total of rows.  (A tile of the strided launch is one item: there is no tile width to exceed.)
QUEUE_RUN = 5


def _queued(method, shape):
    b = LADDER_BOUNDS[shape]

    def call(both, values):
        for v in values:
            both.range_check(0, b, v) if method == "range_check" else both.max_bound(b, v)
            if len(values) >= 2:
                both.boolean_gate(both.zero_var)
    return (lambda both, w, k: [w.randrange(2 * b + 1) for _ in range(k)]), call


def _kind(name, per_shape, shapes, tile, refreshed=True):
    pairs = [per_shape(s) for s in range(shapes)]
    return Kind(name, shapes, tile, lambda both, w, k, s: pairs[s][0](both, w, k), lambda both, ctx, s: pairs[s][1](both, ctx), refreshed)


KINDS = [
    _kind("range_gate_batch", _range_gate, 2, SMALL_TILE),
    _kind("interval_gate_batch", lambda s: _interval(s, False), 2, SMALL_TILE),
    _kind("interval_gate_ragged_batch", lambda s: _interval(s, True), 2, SMALL_TILE),
    _kind("is_less_equal_each", lambda s: _compare(s, False), 2, SMALL_TILE),
    _kind("is_less_equal_each_strict", lambda s: _compare(s, True), 2, SMALL_TILE),
    _kind("weighted_sum_ragged_batch", _weighted_sum, 2, weighted_sum_tile),
    _kind("range_check_batch", lambda s: _ladder("range_check_batch", s), 2, RC_TILE),
    _kind("max_bound_batch", lambda s: _ladder("max_bound_batch", s), 2, MB_TILE),
    _kind("max_bound_ragged_batch", lambda s: _ladder("max_bound_ragged_batch", s, ragged=True), 2, MB_TILE),
    _kind("range_check_ragged_batch", lambda s: _ladder("range_check_ragged_batch", s, ragged=True), 2, RC_TILE),
    _kind("range_check_allocated_batch", lambda s: _ladder("range_check_allocated_batch", s, allocated=True), 2, RC_TILE),
    _kind("max_bound_allocated_batch", lambda s: _ladder("max_bound_allocated_batch", s, allocated=True), 2, RC_TILE),
    _kind("scalar_decomposition_batch", lambda s: _ladder("scalar_decomposition_batch", s, allocated=True), 2, DEC_TILE),
    _kind("conditionally_select_zero_batch", lambda s: _two_inputs("conditionally_select_zero_batch", "bit"), 1, SMALL_TILE),
    _kind("conditionally_select_one_batch", lambda s: _two_inputs("conditionally_select_one_batch", "bit"), 1, SMALL_TILE),
    _kind("maybe_equal_batch", lambda s: _two_inputs("maybe_equal_batch", "equal"), 1, SMALL_TILE),
    _kind("is_non_zero_batch", lambda s: _is_non_zero(False), 1, SMALL_TILE),
    _kind("is_non_zero_batch_failing", lambda s: _is_non_zero(True), 1, SMALL_TILE, refreshed=False),
    _kind("scalar_mix_batch", lambda s: _scalar_mix(False), 1, SMALL_TILE),
    _kind("scalar_mix_batch_failing", lambda s: _scalar_mix(True), 1, SMALL_TILE, refreshed=False),
    _kind("add_batch", lambda s: _gates("add_batch"), 1, SMALL_TILE),
    _kind("mul_batch", lambda s: _gates("mul_batch"), 1, SMALL_TILE),
    _kind("poly_gate_batch", lambda s: _gates("poly_gate_batch"), 1, SMALL_TILE),
    _kind("boolean_gate_batch", lambda s: _gates("boolean_gate_batch"), 1, SMALL_TILE),
    _kind("constrain_to_constant_batch", lambda s: _gates("constrain_to_constant_batch"), 1, SMALL_TILE),
    _kind("add_input_batch", lambda s: _gates("add_input_batch"), 1, SMALL_TILE),
    _kind("queued_range_check", lambda s: _queued("range_check", s), 2, QUEUE_RUN),
    _kind("queued_max_bound", lambda s: _queued("max_bound", s), 2, QUEUE_RUN),
]

# the composers' fixed capacities (rows, Variables): what the program ends at (tests/test_append_alignment_programs.py prints it on
# a failure) and at least cv.ROOM_BEHIND more, rounded up
CAPACITY = {
    "range_gate_batch": (17408, 16384),
    "interval_gate_batch": (28672, 29696),
    "interval_gate_ragged_batch": (28672, 29696),
    "is_less_equal_each": (17408, 25600),
    "is_less_equal_each_strict": (17408, 25600),
    "weighted_sum_ragged_batch": (16384, 30720),
    "range_check_batch": (31744, 686080),
    "max_bound_batch": (14336, 276480),
    "max_bound_ragged_batch": (13312, 276480),
    "range_check_ragged_batch": (30720, 687104),
    "range_check_allocated_batch": (31744, 687104),
    "max_bound_allocated_batch": (17408, 344064),
    "scalar_decomposition_batch": (14336, 343040),
    "conditionally_select_zero_batch": (8192, 14336),
    "conditionally_select_one_batch": (20480, 27648),
    "maybe_equal_batch": (16384, 23552),
    "is_non_zero_batch": (16384, 19456),
    "is_non_zero_batch_failing": (16384, 18432),
    "scalar_mix_batch": (47104, 68608),
    "scalar_mix_batch_failing": (47104, 68608),
    "add_batch": (8192, 14336),
    "mul_batch": (8192, 14336),
    "poly_gate_batch": (8192, 10240),
    "boolean_gate_batch": (8192, 5120),
    "constrain_to_constant_batch": (8192, 5120),
    "add_input_batch": (1024, 5120),
    "queued_range_check": (21504, 449536),
    "queued_max_bound": (13312, 225280),
}


def targets(kind):
    """(row residue, Variable residue, batch, shape) of every call under test, in program order"""
    for r in range(16):
        for v in range(4):
            for shape in range(kind.shapes):
                for batch in BATCHES:
                    yield r, v, batch, shape
    tile = kind.tile
    for r in range(16):
        yield r, r % 4, tile, r % kind.shapes


def label(kind, r, v, batch, shape):
    return f"{kind.name}: shape {shape}, batch {batch} at row residue {r} of 16, Variable residue {v} of 4"


def pad_to(both, r, v):
    zero = both.zero_var
    while both.ora.n % 16 != r:
        both.boolean_gate(zero)
    k = (v - both.ora.num_vars) % 4
    if k:
        both.add_input_batch([1] * k)
    assert both.ora.n % 16 == r and both.ora.num_vars % 4 == v
    if both.dev is not None:
        assert both.dev.circuit_size() % 16 == r and both.dev.num_variables() % 4 == v


class Recorder:
    """the guard of an oracle-only replay: what every guarded call does to the composer's sizes (the device run's plan), and the
    room rule against the kind's fixed capacity"""

    def __init__(self, capacity):
        self.capacity, self.plan = capacity, []

    def around(self, both, what, fn, under_test):
        before = (both.ora.n, both.ora.num_vars)
        fn()
        after = (both.ora.n, both.ora.num_vars)
        cv.room(*(before if under_test else (cv.ROOM_BEFORE_ROWS, cv.ROOM_BEFORE_VARS)), *after, *self.capacity, what)
        self.plan.append((what, before, after))


class DeviceGuard:
    """arm / disarm around every guarded call; the sizes come from the oracle-only replay's plan, so that the room is asserted BEFORE
    the call is made.  keep_rows: the previous build's rows, in the replay after clear_witness"""

    def __init__(self, dev, views, plan, keep_rows=0):
        self.dev, self.views, self.plan, self.keep_rows = dev, views, iter(plan), keep_rows

    def around(self, both, what, fn, under_test):
        planned, before, after = next(self.plan)
        dev = self.dev
        assert planned == what and (dev.circuit_size(), dev.num_variables()) == before, (planned, what)
        cv.room(*(before if under_test else (cv.ROOM_BEFORE_ROWS, cv.ROOM_BEFORE_VARS)), *after, *dev.capacity(), what)
        armed = self.views.arm(dev, self.keep_rows)
        fn()
        self.views.disarm(dev, armed, what, ((before[0], after[0]), (before[1], after[1])))
        assert (dev.circuit_size(), dev.num_variables()) == after, what


def run_program(kind, dev, wit_seed, guard):
    """-> Both; both.calls = [(label, first row, end row, first Variable, end Variable)] of the calls under test"""
    both = AllBoth(dev)
    both.calls = []
    w = random.Random(wit_seed)
    for r, v, batch, shape in targets(kind):
        what = label(kind, r, v, batch, shape)
        ctx = []

        def before():
            ctx.append(kind.prepare(both, w, batch, shape))
            pad_to(both, r, v)
        guard.around(both, "inputs and pads of " + what, before, False)
        n0, v0 = both.ora.n, both.ora.num_vars
        guard.around(both, what, lambda: kind.call(both, ctx[0], shape), True)
        both.calls.append((what, n0, both.ora.n, v0, both.ora.num_vars))
    return both


def replay_on_oracle(kind, wit_seed):
    """-> (Both, plan)"""
    rec = Recorder(CAPACITY[kind.name])
    return run_program(kind, None, wit_seed, rec), rec.plan


def describe(both, column, index):
    """a row (or, for var_values, a Variable) of the whole circuit as call / target alignment / batch, from Both.log and both.calls"""
    variable = column == "var_values"
    for what, n0, n1, v0, v1 in both.calls:
        lo, hi = (v0, v1) if variable else (n0, n1)
        if lo <= index < hi:
            return f"{'Variable' if variable else 'row'} {index - lo} of {hi - lo} of the call {what}"
    if not variable:
        for name, items, num_bits, n0, rows in both.log:
            if n0 <= index < n0 + rows:
                return f"row {index - n0} of {rows} of {name} (a pad or an input of the sweep), items = {items}"
    return "no call under test (an input or a pad of the sweep)"
