"""Builds tests/cpp/libsides_device_ops.so: the test-only harness of csrc/plonk_sides.hpp's transcript replay and fr_from_wide on
the host and on the device (sides_device_ops.hip), with the library's own compiler flags."""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
SRC = os.path.join(HERE, "sides_device_ops.hip")
LIB = os.path.join(HERE, "libsides_device_ops.so")


def build(force: bool = False, out: str = LIB) -> str:
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from plonk_gadgets_amd import build as pg_build
    deps = [SRC] + [os.path.join(pg_build.CSRC, h) for h in ("plonk_sides.hpp", "g1_codec.hpp", "g1.hpp", "fq.hpp", "fr.hpp", "emit.hpp", "experiment.hpp")]
    if not force and os.path.exists(out) and all(os.path.getmtime(d) < os.path.getmtime(out) for d in deps):
        return out
    subprocess.check_call([pg_build.hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-o", out, SRC])
    return out


if __name__ == "__main__":
    print(build(force=True))
