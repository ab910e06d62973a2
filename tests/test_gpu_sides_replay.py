"""GPU: the transcript replay of csrc/plonk_sides.hpp as plonk_sides_kernel runs it -- workgroups of 64 lanes, the sponge in LDS 64
words apart -- from a seed at every sponge position, limb for limb against Python's Transcript set to the same seed
(tests/sides_replay_corpus.py, computed once and shared with tests/test_sides_replay_host.py).  Consecutive lanes stand at
consecutive positions, so every wave permutes at 64 different bytes; one launch has all its lanes at one seed.  And fr_from_wide's
device form against Python integers in two launch shapes.  The harness is tests/cpp/sides_device_ops.hip."""
import numpy as np
import pytest

import sides_replay_corpus as K

pytestmark = pytest.mark.gpu

SHAPES = {"full": 256, "partial_wave": 96}


def dev(raw: bytes):
    import torch
    return torch.frombuffer(bytearray(raw), dtype=torch.uint8).to("cuda:0")


def replay_device(proofs, states, pos, begin):
    import torch
    n = len(pos)
    d = [dev(x) for x in (proofs, states, pos, begin)]
    out = torch.full((n * K.CHALLENGES * 32 + 64,), 0xEE, dtype=torch.uint8, device="cuda:0")
    assert K.harness().sides_replay_device(d[0].data_ptr(), n, d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), out.data_ptr(),
                                           -(-n // 64), 64) == 0
    torch.cuda.synchronize()
    raw = out.cpu().numpy().tobytes()
    assert raw[n * K.CHALLENGES * 32:] == bytes([0xEE]) * 64  # nothing past lane n - 1
    return K.challenges(raw[:n * K.CHALLENGES * 32])


def check(got, want):
    assert len(got) == len(want)
    bad = [(i, k) for i in range(len(want)) for k in range(K.CHALLENGES) if got[i][k] != want[i][k]]
    assert not bad, f"{len(bad)} challenges differ, first (lane, challenge) {bad[0]}"


@pytest.mark.parametrize("n", [332, 1, 63, 65])
def test_device_replay_equals_the_transcript_at_every_seed(n):
    """n = 332: every seed, five full workgroups and one of 12 lanes; 1, 63, 65: a workgroup's edges"""
    proofs, states, pos, begin, want = K.lanes(range(n))
    assert list(pos[:min(n, 166)]) == list(range(min(n, 166)))  # consecutive lanes at consecutive positions
    check(replay_device(proofs, states, pos, begin), want)


def test_device_replay_with_every_lane_at_one_seed():
    """the uniform path: 130 lanes (two workgroups and two lanes) at the seed whose first framing byte ends a block"""
    lane = 166 + 165
    assert K.SEEDS[lane] == (165, 165)
    proofs, states, pos, begin, want = K.lanes([lane] * 130)
    check(replay_device(proofs, states, pos, begin), want)


def test_a_seed_out_of_range_is_not_replayed_on_the_device():
    proofs, states, _, _, _ = K.lanes([0, 1, 2])
    got = replay_device(proofs, states, bytes([166, 5, 255]), bytes([0, 167, 0]))
    assert all(limbs == (2**64 - 1,) * 4 for lane in got for limbs in lane)


@pytest.mark.parametrize("shp", list(SHAPES))
def test_fr_from_wide_on_the_device(shp):
    import torch
    pairs = K.wide_pairs()
    n = len(pairs)
    lo, hi = dev(K.raw256(p[0] for p in pairs)), dev(K.raw256(p[1] for p in pairs))
    out = torch.full((32 * n,), 0xEE, dtype=torch.uint8, device="cuda:0")
    block = SHAPES[shp]
    assert K.harness().fr_from_wide_device(lo.data_ptr(), hi.data_ptr(), out.data_ptr(), n, -(-n // block), block) == 0
    torch.cuda.synchronize()
    got, want = K.limbs256(out.cpu().numpy().astype(np.uint8).tobytes()), K.wide_expected(pairs)
    bad = [i for i in range(n) if got[i] != want[i]]
    assert not bad, f"{len(bad)} of {n} differ, first lo = {hex(pairs[bad[0]][0])}, hi = {hex(pairs[bad[0]][1])}"
