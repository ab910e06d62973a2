"""Times verify_encoded(..., range_term=True) and writes profiles/range_verify_rate.json.  One process:
  row_cost  what the 24th row costs: 2^10 proofs (copies of four proofs) of circuits with NO range items, verify_encoded with and
            without range_term=True in alternation -- after a warm-up of both, three pairs -- both medians and their ratio.  The
            yardstick is the 23-row call of the same process.
  headline  2^10 proofs (copies of four proofs) of small circuits with 64-bit interval_gate items (amounts against per-account
            limits): verify_encoded(range_term=True) beside verify_each on the same proofs -- verify_each once after a warm-up
            call (its subgroup tests then hit their cache), verify_encoded the median of five.
Wall times with the device synchronised before and after.
usage: python tools/range_verify_rate.py [--proofs 1024] [--out profiles/range_verify_rate.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TAU = 0x5EED_7A0 ** 9


def wall(fn, sync):
    sync()
    t = time.perf_counter()
    r = fn()
    sync()
    return (time.perf_counter() - t) * 1e3, r


def spread(ms):
    ms = sorted(ms)
    return {"min": ms[0], "median": ms[len(ms) // 2], "max": ms[-1]}


def proved(pg, comp, ck):
    comp.sync()
    assert comp.check() == -1
    pre = comp.preprocessed_commitments(ck)
    n = 1 << max(0, (comp.circuit_size() - 1).bit_length())
    out = (comp.prove(ck, b"plonk", pre, blinding=True), pg.VerifierKey(n, pre), {})
    comp.close()
    return out


def plain_circuits(pg, eng, ck, count):
    """`count` different small circuits without range items (tools/verify_rate.py's): (proof, verifier key, public inputs)"""
    S = pg.BlsScalar.from_int
    out = []
    for j in range(count):
        comp = pg.StandardComposer(eng, 1 << 12, 1 << 12)
        res = pg.range_check(comp, S(50_000), S(250_000), pg.AllocatedScalar.allocate(comp, S(60_000 + j)))
        comp.constrain_to_constant(res, S(1), None)
        for t in range(j):
            comp.constrain_to_constant(comp.add_input(S(t + 2)), S(t + 2), None)
        out.append(proved(pg, comp, ck))
        assert out[-1][1].commitments["q_range"].is_identity()
    return out


def interval_circuits(pg, eng, ck, count):
    """`count` different small circuits of 64-bit interval_gate items: 4 + j amounts, each within [0, its account's limit]"""
    S = pg.BlsScalar.from_int
    out = []
    for j in range(count):
        comp = pg.StandardComposer(eng, 1 << 12, 1 << 12)
        for k in range(4 + j):
            limit = (1 << 64) - 1 - 1_000_003 * (k + 1)
            comp.interval_gate(comp.add_input(S(limit - 17 * k * (j + 1))), S(0), S(limit), 64)
        out.append(proved(pg, comp, ck))
        assert not out[-1][1].commitments["q_range"].is_identity()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--proofs", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "range_verify_rate.json"))
    args = ap.parse_args()
    import torch
    import plonk_gadgets_amd as pg
    n = args.proofs
    eng = pg.Engine(0)
    sync = lambda: torch.cuda.synchronize()  # noqa: E731
    ck = pg.CommitKey.setup(eng, (1 << 12) - 1, pg.BlsScalar.from_int(TAU))
    ok = pg.OpeningKey.setup(eng, pg.BlsScalar.from_int(TAU))

    def batch(four):
        assert all(p.verify(vk, ok, pi) for p, vk, pi in four)
        proofs, vks, pis = ([four[i % 4][k] for i in range(n)] for k in range(3))
        return proofs, b"".join(four[i % 4][0].to_bytes() for i in range(n)), vks, pis

    # (a) the cost of the 24th row
    _, data, vks, pis = batch(plain_circuits(pg, eng, ck, 4))
    calls = {"rows_23": lambda: pg.verify_encoded(data, vks, ok, pis), "rows_24": lambda: pg.verify_encoded(data, vks, ok, pis, range_term=True)}
    for _ in range(2):  # warm-up: workspaces at both sizes, kernels loaded, the keys' seeds
        assert all(calls["rows_23"]()) and all(calls["rows_24"]())
    ms = {"rows_23": [], "rows_24": []}
    for _ in range(3):
        for name in ("rows_23", "rows_24"):
            t, good = wall(calls[name], sync)
            assert all(good)
            ms[name].append(t)
    row_cost = {"proofs": n, "verify_encoded_ms": spread(ms["rows_23"]), "verify_encoded_range_term_ms": spread(ms["rows_24"]),
                "pairs_ms": [[a, b] for a, b in zip(ms["rows_23"], ms["rows_24"])]}
    row_cost["ratio_of_medians"] = row_cost["verify_encoded_range_term_ms"]["median"] / row_cost["verify_encoded_ms"]["median"]
    print(json.dumps(row_cost), flush=True, file=sys.stderr)

    # (b) the headline, verified
    proofs, data, vks, pis = batch(interval_circuits(pg, eng, ck, 4))
    assert all(pg.verify_encoded(data, vks, ok, pis, range_term=True))
    enc = spread([wall(lambda: pg.verify_encoded(data, vks, ok, pis, range_term=True), sync)[0] for _ in range(5)])
    assert all(pg.verify_each(proofs, vks, ok, pis))
    t_each, good = wall(lambda: pg.verify_each(proofs, vks, ok, pis), sync)
    assert all(good)
    headline = {"proofs": n, "circuit_rows": sorted({vk.n for vk in vks}), "verify_encoded_range_term_ms": enc, "verify_each_ms": t_each,
                "verify_each_over_verify_encoded": t_each / enc["median"]}
    print(json.dumps(headline), flush=True, file=sys.stderr)

    result = {"tool": "range_verify_rate",
              "note": "one process, one build; wall time with the device synchronised; row_cost alternates the two calls on the same "
                      "proofs of circuits without range items (three pairs after a warm-up of both); headline is verify_each once after a "
                      "warm-up call beside the median of five verify_encoded(range_term=True) calls on the same proofs",
              "row_cost": row_cost, "headline": headline}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
