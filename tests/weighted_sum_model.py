"""A model of weighted_sum_ragged_batch in Python integers, independent of the library.

Segment s has the terms b = seg_off[s] .. e = seg_off[s + 1] - 1 (at least two) and states result[s] = k[s] + sum c[t] value(x[t])
by a chain of additions.  With first_row / first_var the call's first row / first new Variable, term t with b < t <= e owns row
first_row + (t - s - 1) and creates Variable first_var + (t - s - 1); a segment's first term owns neither:
  t = b+1:  wires (x[b], x[b+1], new)     (q_m, q_l, q_r, q_o, q_c) = (0, c[b], c[b+1], -1, k[s])
  t > b+1:  wires (new - 1, x[t], new)    (q_m, q_l, q_r, q_o, q_c) = (0, 1,    c[t],   -1, 0)
and the new Variable holds k[s] + sum_{i = b .. t} c[i] value(x[i]) mod r.  result[s] = first_var + seg_off[s + 1] - s - 2."""
from tests import range_gate_model as m

R = m.R


def check_seg_off(seg_off, terms):
    """ValueError naming the first offending segment for what the library refuses"""
    for s in range(len(seg_off) - 1):
        a, b = seg_off[s], seg_off[s + 1]
        if (s == 0 and a != 0) or b - a < 2 or (s == len(seg_off) - 2 and b != terms):
            raise ValueError(f"segment {s}")
    if len(seg_off) == 1 and terms:
        raise ValueError("terms in no segment")


def item(term_vars, values, seg_off, coeffs, constants, first_var):
    """values[t] = the canonical integer term t's Variable holds; coeffs / constants: canonical integers, or None (all 1 / all 0)
    -> (rows, selectors, new_values, results): rows = [(a, b, c)] Variables, selectors = [(q_m, q_l, q_r, q_o, q_c)] integers below r,
    new_values = the canonical integers of the Variables first_var .. the call creates, results = its result Variables"""
    terms, segments = len(term_vars), len(seg_off) - 1
    assert len(values) == terms
    check_seg_off(seg_off, terms)
    c = [1] * terms if coeffs is None else [x % R for x in coeffs]
    k = [0] * segments if constants is None else [x % R for x in constants]
    assert len(c) == terms and len(k) == segments
    rows, sel, new, results = [], [], [], []
    for s in range(segments):
        b, e = seg_off[s], seg_off[s + 1] - 1
        acc = (k[s] + c[b] * values[b]) % R
        for t in range(b + 1, e + 1):
            fresh = first_var + len(new)
            assert fresh == first_var + t - s - 1
            acc = (acc + c[t] * values[t]) % R
            if t == b + 1:
                rows.append((term_vars[b], term_vars[t], fresh))
                sel.append((0, c[b], c[t], R - 1, k[s]))
            else:
                rows.append((fresh - 1, term_vars[t], fresh))
                sel.append((0, 1, c[t], R - 1, 0))
            new.append(acc)
        results.append(first_var + len(new) - 1)
        assert results[-1] == first_var + seg_off[s + 1] - s - 2
    assert len(rows) == terms - segments
    return rows, sel, new, results


def arith_holds(sel, a, b, c):
    q_m, q_l, q_r, q_o, q_c = sel
    return (q_m * a * b + q_l * a + q_r * b + q_o * c + q_c) % R == 0


def closed_form(term_vars, seg_off, first_var):
    """the wires and the segment of every row from the formulas alone (numpy, for calls too long to replay): ->
    (w_l, w_r, w_o, term of the row, segment of the row, first-row mask)"""
    import numpy as np
    seg_off = np.asarray(seg_off, dtype=np.int64)
    x = np.asarray(term_vars, dtype=np.int64)
    terms, segments = len(x), len(seg_off) - 1
    seg_of_term = np.repeat(np.arange(segments, dtype=np.int64), np.diff(seg_off))
    t = np.arange(terms, dtype=np.int64)
    owns = t != seg_off[seg_of_term]
    t, s = t[owns], seg_of_term[owns]
    row = t - s - 1
    assert np.array_equal(row, np.arange(terms - segments))
    first = t == seg_off[s] + 1
    w_o = first_var + row
    w_l = np.where(first, x[t - 1], w_o - 1)
    return w_l, x[t], w_o, t, s, first
