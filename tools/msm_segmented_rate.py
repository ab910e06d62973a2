"""Times pg_msm_segmented alone (csrc/msm_small.hpp) with two scalar columns, warmed up, for
  1 segment of 22 points, 2^10 segments of 27 points, 2^14 segments of 27 points   (--shapes SEGSxLEN,...)
against pg_msm on the first shape, and the fq_mul ceiling re-measured in the same run (tools/fq_mul_bench.hip).  Per shape:
median / min / max ms of --reps calls, Fq products per second by the cost model below, and the fraction of the ceiling.
--lib PATH times another build of the library (the window-width A/B:
  python -c "from plonk_gadgets_amd import build; build.build(force=True, extra_flags=['-DPG_EXPERIMENT', '-DPG_MSM_SMALL_WINDOW=4'],
             out='tools/variants/libpg_msm_small_w4.so')"     and     --lib tools/variants/libpg_msm_small_w4.so --window 4).
Without --phase it is the driver: each phase is a child process under its own time limit, and nothing more is started after a
phase that fails or times out.  One JSON line; --out writes it to a file as well.
usage: python tools/msm_segmented_rate.py [--shapes 1x22,1024x27,16384x27] [--lib PATH --window 4] [--out FILE]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

PHASES = (("ceiling", 120), ("segmented", 300))
DBL, ADD, MADD = 9, 14, 10  # Fq products of g1x_dbl, g1x_add, g1x_add_affine (g1.hpp)


def fq_mul_per_product(window: int) -> int:
    """DESIGN section 3.15's cost model, per point and column: the table (P + P by the complete mixed addition, then mixed
    additions), W doublings under every window but the top one, one addition per window (a wave pays it unless all 64 digits
    are 0), and the product's addition into its segment's sum"""
    windows = 255 // window + 1
    slots = (1 << (window - 1)) - 1
    return (DBL + (slots - 1) * MADD) + (windows - 1) * window * DBL + windows * ADD + ADD


def phase_segmented(shapes, reps, window):
    import numpy as np
    import torch
    import plonk_gadgets_amd as pg
    from plonk_gadgets_amd import synth
    eng = pg.Engine(0)
    biggest = max(s * m for s, m in shapes)
    ck = pg.CommitKey.setup(eng, biggest - 1, pg.BlsScalar.from_int(0x5EED_7A0 ** 9))
    few = torch.from_numpy(synth.uniform_below(1 << 13, synth.Q, seed=15).view(np.int64)).to(eng.device)  # (repeated: timing only)
    sc = few.repeat((2 * biggest + (1 << 13) - 1) >> 13, 1)[:2 * biggest].contiguous().view(2, biggest, 4)
    per = fq_mul_per_product(window)

    def timed(fn):
        ms = []
        for rep in range(reps + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if rep:
                ms.append(e0.elapsed_time(e1))
        ms.sort()
        return {"min": ms[0], "median": ms[len(ms) // 2], "max": ms[-1]}

    rows = []
    for segs, m in shapes:
        n = segs * m
        bases, cols, off = ck.powers[:n], sc[:, :n], list(range(0, n + 1, m))
        t = timed(lambda: eng.msm_segmented(bases, cols, off))
        sec = t["median"] / 1e3
        rows.append({"segments": segs, "points_per_segment": m, "n_cols": 2, "ms": t, "products_per_s": 2 * n / sec,
                     "fq_mul_per_product": per, "fq_mul_per_s": 2 * n * per / sec})
        print(json.dumps(rows[-1]), flush=True, file=sys.stderr)
    segs, m = shapes[0]
    out = {"window": window, "pg_msm_segmented": rows,
           "pg_msm_same_points": {"n": m, "n_cols": 2, "ms": timed(lambda: eng.msm(ck.powers[:m], sc[:, :m]))}}
    eng.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--phase", choices=[p for p, _ in PHASES])
    ap.add_argument("--shapes", default="1x22,1024x27,16384x27")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--window", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    shapes = [tuple(int(v) for v in x.split("x")) for x in args.shapes.split(",") if x]
    if args.phase:
        if args.lib:
            from plonk_gadgets_amd import _lib
            _lib.LIB_PATH = os.path.abspath(args.lib)
        if args.phase == "ceiling":
            import verify_rate
            print(json.dumps(verify_rate.phase_ceiling()))
        else:
            print(json.dumps(phase_segmented(shapes, args.reps, args.window)))
        return
    result = {"tool": "msm_segmented_rate", "library": args.lib or "plonk_gadgets_amd/libplonk_gadgets_hip.so"}
    result.update({p: "unmeasured" for p, _ in PHASES})
    for phase, limit in PHASES:
        cmd = [sys.executable, os.path.abspath(__file__), "--phase", phase, "--shapes", args.shapes, "--reps", str(args.reps),
               "--window", str(args.window)] + (["--lib", args.lib] if args.lib else [])
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            result[phase] = "unmeasured: the phase ran past its %d s limit" % limit
            break
        if p.returncode != 0:
            result[phase] = "unmeasured: the phase failed with status %d: %s" % (p.returncode, p.stderr.strip()[-300:])
            break
        result[phase] = json.loads(p.stdout.strip().split("\n")[-1])
    if isinstance(result["ceiling"], dict) and isinstance(result["segmented"], dict):
        for row in result["segmented"]["pg_msm_segmented"]:
            row["fq_mul_ceiling_fraction"] = row["fq_mul_per_s"] / result["ceiling"]["fq_mul_ceiling_per_s"]
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
