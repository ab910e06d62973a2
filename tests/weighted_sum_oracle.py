"""TEST INFRASTRUCTURE: weighted_sum_ragged_batch replayed on the C oracle's composer, which has no such call:
the loop a user of the reference would write, through composer_add alone, so that the oracle's own bookkeeping gives the columns,
the Variable numbering, check() and sigma.  Both is tests/widget_programs.Both with the call made on either side."""
from oracle import pyoracle as po
from tests import widget_oracle as wo
from tests import widget_programs as wp

F = wo.fr_of
ONE, ZERO = F(1), F(0)


def replay(ora, term_vars, seg_off, coeffs=None, constants=None):
    """-> the result Variables"""
    L, c = ora.L, ora.c
    x = [int(v) for v in term_vars]
    co = [ONE] * len(x) if coeffs is None else [F(v) for v in coeffs]
    results = []
    for s in range(len(seg_off) - 1):
        b, e = seg_off[s], seg_off[s + 1] - 1
        assert e - b + 1 >= 2
        acc = L.composer_add(c, co[b], x[b], co[b + 1], x[b + 1], ZERO if constants is None else F(constants[s]), None)
        for t in range(b + 2, e + 1):
            acc = L.composer_add(c, ONE, acc, co[t], x[t], ZERO, None)
        results.append(int(acc))
    return results


class Both(wp.Both):
    def weighted_sum_ragged_batch(self, term_vars, seg_off, coeffs=None, constants=None, want_results=True):
        n0 = self.ora.n
        r = None
        if self.dev is not None:
            args = (self.tv(term_vars), self.tv(seg_off), None if coeffs is None else self.t(coeffs),
                    None if constants is None else self.t(constants))
            if want_results:
                r = self.dev.weighted_sum_ragged_batch(*args)
            else:      # d_result_vars = NULL: the C call itself
                h = self.dev._lib.pg_composer_weighted_sum_ragged_batch
                assert h(self.dev._h, args[0].data_ptr(), args[1].data_ptr(), None if args[2] is None else args[2].data_ptr(),
                         None if args[3] is None else args[3].data_ptr(), len(term_vars), len(seg_off) - 1, None) == 0
        o = replay(self.ora, term_vars, seg_off, coeffs, constants)
        if r is not None:
            self._same_vars(r, o)
        self._logged("weighted_sum_ragged_batch", len(seg_off) - 1, None, n0)
        return o


# ---- the cases both suites run ------------------------------------------------------------------------------------------------
R = wp.R
ZV = -1     # in a case's `terms`: the composer's zero_var


def _case(name, inputs, terms, seg_off, coeffs=None, constants=None):
    return dict(name=name, inputs=[v % R for v in inputs], terms=list(terms), seg_off=list(seg_off), coeffs=coeffs, constants=constants)


def cases():
    """inputs: values allocated first; terms: indices into them (ZV: zero_var); seg_off, coeffs, constants as the call takes them"""
    import random
    rng = random.Random(322)
    out = []
    sizes = (2, 3, 17, 300, 2, 5)
    n = sum(sizes)
    off = [0]
    for m in sizes:
        off.append(off[-1] + m)
    vals = [rng.choice([0, 1, rng.randrange(1 << 64), rng.randrange(R)]) for _ in range(40)]
    terms = [rng.randrange(40) for _ in range(n)]
    co = [rng.choice([0, 1, R - 1, rng.randrange(R)]) for _ in range(n)]
    ks = [0, R - 1, rng.randrange(R), 5, 0, R - 1]
    for with_c in (False, True):
        for with_k in (False, True):
            out.append(_case(f"sizes_2_3_17_300{'_coeffs' if with_c else ''}{'_constants' if with_k else ''}", vals, terms, off,
                             co if with_c else None, ks if with_k else None))
    # a Variable twice in one segment, in positions 0 and 1: row 0 has a == b
    out.append(_case("same_variable_twice", [7, 9], [0, 0, 1, 1, 1, 0], [0, 3, 6], [3, 4, 5, R - 1, 1, 0], [1, 2]))
    out.append(_case("zero_var_as_a_term", [11, 13], [ZV, 0, 1, ZV, ZV, 0, ZV], [0, 2, 5, 7], [5, 1, 1, 9, 0, 1, R - 1], None))
    out.append(_case("edge_coefficients_and_constants", [R - 1, 1, 2, R - 2], [0, 1, 2, 3, 0, 1, 2, 3], [0, 4, 6, 8],
                     [0, 1, R - 1, R - 1, R - 1, R - 1, 0, 0], [0, R - 1, R - 1]))
    # sums that are exactly 0 mod r: 5 - 5, (r - 3) + 3, 2 * 4 + (r - 8) from the constant
    out.append(_case("sum_exactly_zero", [5, R - 3, 3, 4], [0, 0, 1, 2, 3, 3], [0, 2, 4, 6], [1, R - 1, 1, 1, 1, 1], [0, 0, R - 8]))
    return out


def run_case(both, case):
    """allocate the case's inputs and make its call -> (term Variables, first row, first new Variable, result Variables)"""
    vs = both.add_input_batch(case["inputs"])
    x = [both.zero_var if i == ZV else vs[i] for i in case["terms"]]
    n0, v0 = both.ora.n, both.ora.num_vars
    res = both.weighted_sum_ragged_batch(x, case["seg_off"], case["coeffs"], case["constants"])
    return x, n0, v0, res
