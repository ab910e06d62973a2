"""Times the verifier (DESIGN sections 3.13 and 3.15) and writes profiles/r15_verify_rate.json (profiles/r13_verify_rate.json is the
run of section 3.13, before pg_msm_segmented, and stays as it is):
  single   one verify of a range_check circuit's proof, split into transcript (the host side: subgroup tests, challenges, the
           two columns of coefficients), MSM (the one two-column pg_msm; beside it the same table as ONE segment of
           pg_msm_segmented) and pairing (one pg_pairing_check of 1 x 2)
  batch    verify_batch and verify_each at --sizes proofs (default 2^6, 2^10, 2^14; copies of four circuits' proofs, so the
           subgroup tests hit their cache after the first four: the host's share is reported apart); up to --per-proof-max
           proofs also verify_each as it was before pg_msm_segmented, one pg_msm per proof (verify_each_per_proof_msm_ms)
  encoded  verify_encoded (the sides built on the device from proof bytes) beside verify_each on the SAME
           proofs at --encoded-sizes (default 1, 2^6, 2^10; verify_encoded alone also at 2^14): medians of 5 warmed-up calls with
           min and max, verify_each's host share (verifier.sides over the batch, 3 calls) measured in the same process, and
           pg_plonk_sides alone between two events.  profiles/r16_verify_encoded.json is this phase's file, made by two commands:
             rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o enc -- python tools/verify_rate.py --phase encoded-trace
             python tools/verify_rate.py --phase encoded --kernel-stats DIR/enc_kernel_stats.csv --out profiles/r16_verify_encoded.json
           (encoded-trace: four verify_encoded calls of 2^10 proofs and nothing timed, the process the trace wraps; with --out the
           encoded phase writes its rows, and the per-call figures of its five kernels from --kernel-stats, instead of printing)
  pairing  pg_pairing_check alone at --checks n_checks (default 1, 2^10, 2^14, 2^16) of two pairs: ms, checks/s, and the
           cost model's Fq products per check (FQ_MUL_PER_CHECK) per second over the fq_mul ceiling
  ceiling  tools/fq_mul_bench.hip re-measured in the same run (built with hipcc if the binary is missing)
  model    for scale, tests/pairing_model.py's time for one pairing on this host
Without --phase it is the driver: every phase runs as a child process of its own under its own time limit, in that order, and
the driver stops at the first phase that fails or times out (nothing more is started on the GPU after a fault); phases that did
not run stay "unmeasured" in the JSON.  With --phase NAME it runs that phase and prints its JSON.
usage: python tools/verify_rate.py [--sizes 64,1024,16384] [--checks 1,1024,16384,65536] [--out profiles/r15_verify_rate.json]"""
import argparse
import json
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

FQ_MUL_CEILING = 3.78e10  # profiles/r11_fq_mul_bench.txt; replaced by the `ceiling` phase's figure when that ran
# DESIGN section 3.13's cost model, Fq products per check of n_pairs pairs
MILLER_SQUARINGS, LINES, PRODUCT, SPARSE_PER_LANE = 63, 68, 108, 10
EASY, HARD = 950, 5 * 68 * 108 + 9 * 108
PHASES = (("ceiling", 120), ("model", 120), ("single", 300), ("pairing", 300), ("batch", 900), ("encoded", 600))
TAU = 0x5EED_7A0 ** 9


def fq_mul_per_check(n_pairs: int) -> int:
    return MILLER_SQUARINGS * PRODUCT + LINES * n_pairs * 6 * SPARSE_PER_LANE + EASY + HARD


def circuits(pg, eng, ck, count):
    """`count` different small circuits: (proof, verifier key, public inputs)"""
    S = pg.BlsScalar.from_int
    out = []
    for j in range(count):
        comp = pg.StandardComposer(eng, 1 << 12, 1 << 12)
        res = pg.range_check(comp, S(50_000), S(250_000), pg.AllocatedScalar.allocate(comp, S(60_000 + j)))
        comp.constrain_to_constant(res, S(1), None)
        for t in range(j):
            comp.constrain_to_constant(comp.add_input(S(t + 2)), S(t + 2), None)
        comp.sync()
        pre = comp.preprocessed_commitments(ck)
        n = 1 << max(0, (comp.circuit_size() - 1).bit_length())
        out.append((comp.prove(ck, b"plonk", pre), pg.VerifierKey(n, pre), {}))
        comp.close()
    return out


def wall(fn, sync):
    sync()
    t = time.perf_counter()
    r = fn()
    sync()
    return (time.perf_counter() - t) * 1e3, r


def phase_single():
    import torch
    import plonk_gadgets_amd as pg
    from plonk_gadgets_amd import verifier as V
    eng = pg.Engine(0)
    sync = lambda: torch.cuda.synchronize()  # noqa: E731
    ck = pg.CommitKey.setup(eng, (1 << 12) - 1, pg.BlsScalar.from_int(TAU))
    ok = pg.OpeningKey.setup(eng, pg.BlsScalar.from_int(TAU))
    proof, vk, pi = circuits(pg, eng, ck, 1)[0]
    assert proof.verify(vk, ok, pi)  # warm-up: MSM workspace, kernels loaded
    rows = []
    for cold in (True, False):
        if cold:
            V._valid_limbs.cache_clear()
        t_tr, table = wall(lambda: V.sides(proof, vk, ok, pi), sync)
        t_msm, ab = wall(lambda: V._msm2(eng, table), sync)
        t_seg, seg = wall(lambda: V._msm2_segmented(eng, [table]), sync)
        assert pg.g1.points_of(seg[0]) == list(ab)
        t_pair, good = wall(lambda: V._check(eng, ok, [tuple(ab)]), sync)
        assert good == [True]
        rows.append({"subgroup_cache": "cold" if cold else "warm", "transcript_ms": t_tr, "msm_ms": t_msm, "msm_segmented_ms": t_seg,
                     "pairing_ms": t_pair, "total_ms": t_tr + t_msm + t_pair, "total_segmented_ms": t_tr + t_seg + t_pair,
                     "msm_points": len(table)})
    return {"verify": rows}


def each_per_proof(V, proofs, vks, ok, pis):
    """verify_each as it was before pg_msm_segmented: one two-column pg_msm per proof, then one pg_pairing_check"""
    pairs = [tuple(V._msm2(ok.engine, V.sides(p, vk, ok, pi))) for p, vk, pi in zip(proofs, vks, pis)]
    return V._check(ok.engine, ok, pairs)


def phase_batch(sizes, per_proof_max):
    import torch
    import plonk_gadgets_amd as pg
    from plonk_gadgets_amd import verifier as V
    eng = pg.Engine(0)
    sync = lambda: torch.cuda.synchronize()  # noqa: E731
    ck = pg.CommitKey.setup(eng, (1 << 12) - 1, pg.BlsScalar.from_int(TAU))
    ok = pg.OpeningKey.setup(eng, pg.BlsScalar.from_int(TAU))
    four = circuits(pg, eng, ck, 4)
    assert all(p.verify(vk, ok, pi) for p, vk, pi in four)
    rows = []
    for n in sizes:
        proofs, vks, pis = ([four[i % 4][k] for i in range(n)] for k in range(3))
        t_host, tables = wall(lambda: [V.sides(p, vk, ok, pi) for p, vk, pi in zip(proofs, vks, pis)], sync)
        t_batch, good = wall(lambda: pg.verify_batch(proofs, vks, ok, pis), sync)
        assert good
        row = {"proofs": n, "host_sides_ms": t_host, "verify_batch_ms": t_batch, "verify_batch_proofs_per_s": n / t_batch * 1e3}
        print(json.dumps(row), flush=True, file=sys.stderr)
        t_each, goods = wall(lambda: pg.verify_each(proofs, vks, ok, pis), sync)
        assert all(goods)
        row.update({"verify_each_ms": t_each, "verify_each_proofs_per_s": n / t_each * 1e3})
        if n <= per_proof_max:
            t_old, goods = wall(lambda: each_per_proof(V, proofs, vks, ok, pis), sync)
            assert all(goods)
            row["verify_each_per_proof_msm_ms"] = t_old
        rows.append(row)
    return {"batches": rows}


def spread(ms):
    ms = sorted(ms)
    return {"min": ms[0], "median": ms[len(ms) // 2], "max": ms[-1]}


def phase_encoded(sizes, alone_sizes):
    import torch
    import plonk_gadgets_amd as pg
    from plonk_gadgets_amd import verifier as V
    eng = pg.Engine(0)
    sync = lambda: torch.cuda.synchronize()  # noqa: E731
    ck = pg.CommitKey.setup(eng, (1 << 12) - 1, pg.BlsScalar.from_int(TAU))
    ok = pg.OpeningKey.setup(eng, pg.BlsScalar.from_int(TAU))
    four = circuits(pg, eng, ck, 4)
    assert all(p.verify(vk, ok, pi) for p, vk, pi in four)
    encoded = [p.to_bytes() for p, _, _ in four]
    rows = []
    for n in sorted(set(sizes) | set(alone_sizes)):
        proofs, vks, pis = ([four[i % 4][k] for i in range(n)] for k in range(3))
        data = b"".join(encoded[i % 4] for i in range(n))
        assert all(pg.verify_encoded(data, vks, ok, pis))  # warm-up: workspaces, kernels loaded, the keys' seeds
        row = {"proofs": n, "verify_encoded_ms": spread([wall(lambda: pg.verify_encoded(data, vks, ok, pis), sync)[0] for _ in range(5)])}
        # pg_plonk_sides alone: everything uploaded, two events around the call
        d_proofs = torch.frombuffer(bytearray(data), dtype=torch.uint8).to(eng.device)
        records = {id(vk): vk.record(ok) for vk in vks}
        d_keys = torch.frombuffer(bytearray(b"".join(records.values())), dtype=torch.uint8).to(eng.device)
        index = torch.tensor([list(records).index(id(vk)) for vk in vks], dtype=torch.int32, device=eng.device)
        ms = []
        for rep in range(6):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            status = eng.plonk_sides(d_proofs, d_keys, index)[2]
            e1.record()
            sync()
            if rep:
                ms.append(e0.elapsed_time(e1))
        assert not bool(status.any())
        row["pg_plonk_sides_ms"] = spread(ms)
        if n in sizes:
            assert all(pg.verify_each(proofs, vks, ok, pis))
            row["verify_each_ms"] = spread([wall(lambda: pg.verify_each(proofs, vks, ok, pis), sync)[0] for _ in range(5)])
            row["verify_each_host_sides_ms"] = spread([wall(lambda: [V.sides(p, vk, ok, pi) for p, vk, pi in zip(proofs, vks, pis)],
                                                            sync)[0] for _ in range(3)])
            row["verify_each_over_verify_encoded"] = row["verify_each_ms"]["median"] / row["verify_encoded_ms"]["median"]
            row["encoded_below_host_share"] = row["verify_encoded_ms"]["median"] < row["verify_each_host_sides_ms"]["median"]
        print(json.dumps(row), flush=True, file=sys.stderr)
        rows.append(row)
    return {"encoded": rows}


def phase_encoded_trace():
    import torch
    import plonk_gadgets_amd as pg
    eng = pg.Engine(0)
    ck = pg.CommitKey.setup(eng, (1 << 12) - 1, pg.BlsScalar.from_int(TAU))
    ok = pg.OpeningKey.setup(eng, pg.BlsScalar.from_int(TAU))
    four = circuits(pg, eng, ck, 4)
    n = 1024
    data = b"".join(four[i % 4][0].to_bytes() for i in range(n))
    vks, pis = [four[i % 4][1] for i in range(n)], [four[i % 4][2] for i in range(n)]
    for _ in range(4):
        assert all(pg.verify_encoded(data, vks, ok, pis))
    torch.cuda.synchronize()
    return {"encoded_trace": {"proofs": n, "calls": 4}}


ENCODED_KERNELS = ("plonk_sides_decode_kernel", "plonk_sides_kernel", "msm_seg_mul_kernel", "msm_seg_sum_kernel", "pairing_check_kernel")


def encoded_profile(rows, kernel_stats=None):
    """the content of profiles/r16_verify_encoded.json: the encoded phase's rows and, from the kernel-stats CSV of a rocprofv3 run
    around the encoded-trace phase, the per-call figures of verify_encoded's five kernels"""
    out = {"tool": "verify_rate --phase encoded",
           "note": "one session, one build; verify_each is the host-sides path on the same proofs (copies of four circuits' proofs, so its "
                   "subgroup tests hit their cache); medians of 5 warmed-up calls (host sides: 3), wall time with the device synchronised; "
                   "pg_plonk_sides_ms between two events with everything uploaded",
           "encoded": rows}
    if kernel_stats:
        import csv
        trace = {}
        for r in csv.DictReader(open(kernel_stats)):
            for k in ENCODED_KERNELS:
                if "pg::" + k + "(" in r["Name"]:
                    trace[k] = {"calls": int(r["Calls"]), "average_ms": float(r["AverageNs"]) / 1e6, "min_ms": int(r["MinNs"]) / 1e6,
                                "max_ms": int(r["MaxNs"]) / 1e6}
        out["kernel_trace_2_10_proofs"] = {
            "how": "rocprofv3 --kernel-trace --stats (no counters) around `verify_rate.py --phase encoded-trace`: four verify_encoded calls of "
                   "2^10 proofs; the other kernels of that process belong to its setup (SRS, proving the four circuits); merged into this "
                   "file by `verify_rate.py --phase encoded --kernel-stats CSV --out FILE` (the file as first recorded was put together by "
                   "encoded_profile() from that phase's printed rows and the CSV of a trace around a script with encoded-trace's body)", "per_call": trace}
    return out


def phase_pairing(checks):
    import torch
    import plonk_gadgets_amd as pg
    import g1_model as G
    eng = pg.Engine(0)
    S = pg.BlsScalar.from_int
    b = 0x5EED
    h = pg.G2Affine.generator()
    prep = [pg.PreparedG2(eng, h.mul(S(b))), pg.PreparedG2(eng, h)]
    R = pg.transcript.R
    pairs = []
    for a in range(3, 11):
        pairs += [pg.G1Affine.from_ints(*G.mul(a, G.G)), pg.G1Affine.from_ints(*G.mul((-a * b) % R, G.G))]
    eight = pg.g1.points_tensor(pairs, eng.device).view(8, 2, 12)
    per_check = fq_mul_per_check(2)
    rows = []
    for n in checks:
        pts = eight.repeat((n + 7) // 8, 1, 1)[:n].contiguous()
        ms = []
        for rep in range(4):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = pg.pairing_check(eng, pts, prep)
            e1.record()
            torch.cuda.synchronize()
            if rep:
                ms.append(e0.elapsed_time(e1))
        assert bool(out.all())
        ms.sort()
        sec = ms[len(ms) // 2] / 1e3
        rows.append({"n_checks": n, "n_pairs": 2, "ms": {"min": ms[0], "median": ms[len(ms) // 2], "max": ms[-1]}, "checks_per_s": n / sec,
                     "fq_mul_per_check": per_check, "fq_mul_per_s": n * per_check / sec})
    return {"pairing_check": rows}


def phase_ceiling():
    exe = os.path.join(ROOT, "tools", "fq_mul_bench")
    if not os.path.exists(exe):
        from plonk_gadgets_amd import build as pg_build
        subprocess.check_call([pg_build.hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-o", exe, exe + ".hip"])
    text = subprocess.run([exe], capture_output=True, text=True, check=True, timeout=100).stdout
    m = re.search(r"variant 1 .*?([0-9.]+e[+-]?\d+) fq-mul/s", text)
    return {"fq_mul_ceiling_per_s": float(m.group(1)), "fq_mul_bench": text.strip().split("\n")}


def phase_model():
    import g1_model as G
    import pairing_model as M
    t = time.perf_counter()
    f = M.miller_loop([(G.G, M.g2_prepare(M.G2))])
    t_miller = time.perf_counter() - t
    t = time.perf_counter()
    M.final_exponentiation_plain(f)
    t_plain = time.perf_counter() - t
    t = time.perf_counter()
    M.final_exponentiation_chain(f)
    t_chain = time.perf_counter() - t
    return {"python_model_one_pairing_ms": {"prepare_and_miller": t_miller * 1e3, "final_plain_power": t_plain * 1e3,
                                            "final_chain": t_chain * 1e3}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--phase", choices=[p for p, _ in PHASES] + ["encoded-trace"])
    ap.add_argument("--kernel-stats", help="with --phase encoded --out: a rocprofv3 kernel-stats CSV of the encoded-trace phase to merge")
    ap.add_argument("--sizes", default="64,1024,16384")
    ap.add_argument("--checks", default="1,1024,16384,65536")
    ap.add_argument("--per-proof-max", type=int, default=1024)
    ap.add_argument("--encoded-sizes", default="1,64,1024")
    ap.add_argument("--encoded-alone-sizes", default="16384")
    ap.add_argument("--out", help="default for a full run: profiles/r15_verify_rate.json; with --phase encoded: that phase's file")
    args = ap.parse_args()
    sizes = [int(x) for x in args.sizes.split(",") if x]
    checks = [int(x) for x in args.checks.split(",") if x]
    enc_sizes, enc_alone = ([int(x) for x in v.split(",") if x] for v in (args.encoded_sizes, args.encoded_alone_sizes))
    if args.phase:
        fn = {"single": phase_single, "batch": lambda: phase_batch(sizes, args.per_proof_max), "pairing": lambda: phase_pairing(checks),
              "ceiling": phase_ceiling, "model": phase_model, "encoded": lambda: phase_encoded(enc_sizes, enc_alone),
              "encoded-trace": phase_encoded_trace}[args.phase]
        res = fn()
        if args.phase == "encoded" and args.out:
            with open(args.out, "w") as f:
                json.dump(encoded_profile(res["encoded"], args.kernel_stats), f, indent=1)
                f.write("\n")
        print(json.dumps(res))
        return
    args.out = args.out or os.path.join(ROOT, "profiles", "r15_verify_rate.json")
    result = {"tool": "verify_rate", "fq_mul_per_check_two_pairs": fq_mul_per_check(2), "fq_mul_ceiling_per_s": FQ_MUL_CEILING,
              "fq_mul_ceiling_source": "profiles/r11_fq_mul_bench.txt"}
    result.update({p: "unmeasured" for p, _ in PHASES})
    for phase, limit in PHASES:
        cmd = [sys.executable, os.path.abspath(__file__), "--phase", phase, "--sizes", args.sizes, "--checks", args.checks,
               "--per-proof-max", str(args.per_proof_max), "--encoded-sizes", args.encoded_sizes, "--encoded-alone-sizes",
               args.encoded_alone_sizes]
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            result[phase] = "unmeasured: the phase ran past its %d s limit" % limit
            break
        if p.returncode != 0:
            result[phase] = "unmeasured: the phase failed with status %d: %s" % (p.returncode, p.stderr.strip()[-300:])
            break
        result[phase] = json.loads(p.stdout.strip().split("\n")[-1])
        if phase == "ceiling":
            result["fq_mul_ceiling_per_s"] = result[phase]["fq_mul_ceiling_per_s"]
            result["fq_mul_ceiling_source"] = "tools/fq_mul_bench.hip, this run"
    if isinstance(result["pairing"], dict):
        for row in result["pairing"]["pairing_check"]:
            row["fq_mul_ceiling_fraction"] = row["fq_mul_per_s"] / result["fq_mul_ceiling_per_s"]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
