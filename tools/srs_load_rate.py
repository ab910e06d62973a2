"""Times G1 ingestion and writes profiles/r14_srs_load_rate.json:
  ceiling     tools/fq_mul_bench.hip re-measured in the same run (built with hipcc if the binary is missing)
  codec       at --sizes points (default 2^20, 2^24, 2^26; the powers of a development key): pg_g1_decompress with and without
              the membership test, pg_g1_check alone, pg_g1_compress -- ms, points/s, and the cost model's Fq products per
              point per second over the fq_mul ceiling
  consistent  PublicParameters.is_consistent at the same sizes, split into drawing the scalars and the rest (two MSMs, a check)
  load        CommitKey.load of a file of --load-points powers (default 2^24; just written, so read from the page cache) with the
              checks on, beside the decode + check of the same points already on the device and the upload of one 48-MiB chunk
              alone: what the fetch and the upload gap of the one-buffer pipeline cost
The ceiling phase also runs the bench at one workgroup of 256 per CU -- one wave per SIMD, the occupancy of the two heavy kernels.
Without --phase it is the driver: every phase runs as a child process of its own under its own `timeout -k 10`, in that order,
and the driver stops at the first phase that fails or times out (nothing more is started on the GPU after a fault); phases that
did not run stay "unmeasured" in the JSON.  With --phase NAME it runs that phase and prints its JSON.
usage: python tools/srs_load_rate.py [--sizes 1048576,16777216,67108864] [--load-points 16777216]
       [--out profiles/r14_srs_load_rate.json]"""
import argparse
import json
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FQ_MUL_CEILING = 3.78e10  # profiles/r11_fq_mul_bench.txt; replaced by the `ceiling` phase's figure when that ran
# DESIGN section 3.14's cost model, Fq products per point
SQRT = 2 + 378 + 156                      # x^2 and x^3 of the window, the squarings, the window's products (the first assigns)
DECODE = 1 + 2 + SQRT + 1 + 1             # to Montgomery form, x^3, the root, y^2, the sign's reduction
MEMBER = 2 * (63 * 9 + 5 * 14) + 4        # [|u|][|u|] P by complete XYZZ steps, beta x ZZ and y ZZZ
ON_CURVE = 3
ENCODE = 2                                # two reductions out of Montgomery form (a reduction counted as a product)
FQ_MUL = {"decompress_check": DECODE + MEMBER, "decompress": DECODE, "check": ON_CURVE + MEMBER, "compress": ENCODE}
PHASES = (("ceiling", 120), ("codec", 600), ("consistent", 600), ("load", 600))
TAU = 0x5EED_7A0 ** 9


def timed(fn, reps=3):
    import torch
    ms = []
    for rep in range(reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        if rep:
            ms.append(e0.elapsed_time(e1))
    ms.sort()
    return ms, out


def phase_codec(sizes):
    import torch
    import plonk_gadgets_amd as pg
    eng = pg.Engine(0)
    rows = []
    for n in sizes:
        key = pg.CommitKey.setup(eng, n - 1, pg.BlsScalar.from_int(TAU))
        data = eng.g1_compress(key.powers).view(-1)
        out = torch.empty_like(key.powers)
        row = {"points": n}
        calls = {"decompress_check": lambda: eng._g1_decompress_into(data, True, out),
                 "decompress": lambda: eng._g1_decompress_into(data, False, out),
                 "check": lambda: eng._g1_check(key.powers),
                 "compress": lambda: eng.g1_compress(key.powers)}
        for name, fn in calls.items():
            ms, res = timed(fn)
            if name != "compress":
                assert int(res[1].item()) == n, (name, int(res[1].item()))
            if name.startswith("decompress"):
                assert torch.equal(out, key.powers)
            sec = ms[len(ms) // 2] / 1e3
            row[name] = {"ms": {"min": ms[0], "median": ms[len(ms) // 2], "max": ms[-1]}, "points_per_s": n / sec,
                         "fq_mul_per_point": FQ_MUL[name], "fq_mul_per_s": n * FQ_MUL[name] / sec}
        print(json.dumps(row), flush=True, file=sys.stderr)
        rows.append(row)
        del key, data, out
        torch.cuda.empty_cache()
    return {"codec": rows}


def phase_consistent(sizes):
    import torch
    import plonk_gadgets_amd as pg
    eng = pg.Engine(0)
    rows = []
    for n in sizes:
        pp = pg.PublicParameters.setup(eng, n - 1, pg.BlsScalar.from_int(TAU))
        torch.cuda.synchronize()
        t = time.perf_counter()
        pp._random_scalars(n - 1)
        torch.cuda.synchronize()
        t_rho = time.perf_counter() - t
        times = []
        for rep in range(2):
            t = time.perf_counter()
            good = pp.is_consistent()
            times.append(time.perf_counter() - t)
            assert good
        row = {"points": n, "is_consistent_ms": min(times) * 1e3, "first_call_ms": times[0] * 1e3, "of_which_scalars_ms": t_rho * 1e3}
        print(json.dumps(row), flush=True, file=sys.stderr)
        rows.append(row)
        pp.opening_key.close()
        del pp
        torch.cuda.empty_cache()
    return {"is_consistent": rows}


def phase_ceiling():
    exe = os.path.join(ROOT, "tools", "fq_mul_bench")
    if not os.path.exists(exe):
        from plonk_gadgets_amd import build as pg_build
        subprocess.check_call([pg_build.hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-o", exe, exe + ".hip"])
    out = {}
    # the default shape (2048 workgroups of 256: the ceiling), then one workgroup per CU
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    for key, shape in (("fq_mul_ceiling_per_s", []), ("fq_mul_one_wave_per_simd_per_s", [str(cus), "256"])):
        text = subprocess.run([exe] + shape, capture_output=True, text=True, check=True, timeout=100).stdout
        m = re.search(r"variant 1 .*?([0-9.]+e[+-]?\d+) fq-mul/s", text)
        if m is None:
            raise SystemExit("fq_mul_bench printed no 'variant 1 ... fq-mul/s' line:\n" + text)
        out[key] = float(m.group(1))
        out.setdefault("fq_mul_bench", []).extend(text.strip().split("\n"))
    out["compute_units"] = cus
    return out


def phase_load(n):
    import tempfile
    import torch
    import plonk_gadgets_amd as pg
    from plonk_gadgets_amd.g1 import LOAD_CHUNK
    eng = pg.Engine(0)
    key = pg.CommitKey.setup(eng, n - 1, pg.BlsScalar.from_int(TAU))
    data = eng.g1_compress(key.powers).view(-1)
    out = torch.empty_like(key.powers)
    ms_dev, _ = timed(lambda: eng._g1_decompress_into(data, True, out))
    m = 48 * min(LOAD_CHUNK, n)
    pinned = torch.empty((m,), dtype=torch.uint8).pin_memory()
    staged = torch.empty((m,), dtype=torch.uint8, device=eng.device)
    ms_up, _ = timed(lambda: staged.copy_(pinned, non_blocking=True), reps=5)
    row = {"points": n, "chunk_points": min(LOAD_CHUNK, n), "chunks": (n + LOAD_CHUNK - 1) // LOAD_CHUNK,
           "decompress_check_on_device_ms": ms_dev[len(ms_dev) // 2], "upload_one_chunk_ms": ms_up[len(ms_up) // 2],
           "upload_one_chunk_bytes": m}
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "ck.bin")
        t = time.perf_counter()
        key.save(path)
        row["save_ms"] = (time.perf_counter() - t) * 1e3
        t = time.perf_counter()
        with open(path, "rb") as f:
            while f.readinto(memoryview(pinned.numpy())):
                pass
        row["read_file_alone_ms"] = (time.perf_counter() - t) * 1e3
        times = []
        for rep in range(3):
            torch.cuda.synchronize()
            t = time.perf_counter()
            back = pg.CommitKey.load(eng, path)
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t) * 1e3)
        assert torch.equal(back.powers, key.powers)
    times.sort()
    row["load_ms"] = {"min": times[0], "median": times[1], "max": times[-1]}
    row["load_points_per_s"] = n / times[1] * 1e3
    row["load_over_device_decode"] = times[1] / row["decompress_check_on_device_ms"]
    return {"load": row}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--phase", choices=[p for p, _ in PHASES])
    ap.add_argument("--sizes", default="1048576,16777216,67108864")
    ap.add_argument("--load-points", type=int, default=1 << 24)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14_srs_load_rate.json"))
    args = ap.parse_args()
    sizes = [int(x) for x in args.sizes.split(",") if x]
    if args.phase:
        fn = {"codec": lambda: phase_codec(sizes), "consistent": lambda: phase_consistent(sizes), "ceiling": phase_ceiling,
              "load": lambda: phase_load(args.load_points)}[args.phase]
        print(json.dumps(fn()))
        return
    result = {"tool": "srs_load_rate", "fq_mul_per_point": FQ_MUL, "fq_mul_ceiling_per_s": FQ_MUL_CEILING,
              "fq_mul_ceiling_source": "profiles/r11_fq_mul_bench.txt"}
    result.update({p: "unmeasured" for p, _ in PHASES})
    for phase, limit in PHASES:
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--phase", phase, "--sizes", args.sizes,
               "--load-points", str(args.load_points)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)  # (stderr passes through: the phases' progress lines)
        if p.returncode in (124, 137):
            result[phase] = "unmeasured: the phase ran past its %d s limit" % limit
            break
        if p.returncode != 0:
            result[phase] = "unmeasured: the phase failed with status %d" % p.returncode
            break
        result[phase] = json.loads(p.stdout.strip().split("\n")[-1])
        if phase == "ceiling":
            result["fq_mul_ceiling_per_s"] = result[phase]["fq_mul_ceiling_per_s"]
            result["fq_mul_ceiling_source"] = "tools/fq_mul_bench.hip, this run"
            result["fq_mul_one_wave_per_simd_per_s"] = result[phase]["fq_mul_one_wave_per_simd_per_s"]
    if isinstance(result["codec"], dict):
        for row in result["codec"]["codec"]:
            for name in FQ_MUL:
                row[name]["fq_mul_ceiling_fraction"] = row[name]["fq_mul_per_s"] / result["fq_mul_ceiling_per_s"]
                if "fq_mul_one_wave_per_simd_per_s" in result:
                    row[name]["fraction_of_one_wave_per_simd_rate"] = row[name]["fq_mul_per_s"] / result["fq_mul_one_wave_per_simd_per_s"]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
