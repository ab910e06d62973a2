"""GPU: commit keys and public parameters to bytes and back (plonk_gadgets_amd.g1.CommitKey, plonk_gadgets_amd.srs).

Round trips against the model's encodings and bit for bit on the powers tensor (1, 2, 2^10 + 3 and 2^20 powers; files with a
chunk boundary inside; a prefix by max_degree); a range_check circuit proved under a key LOADED from a file -- no tau in sight --
with the proof's bytes equal to those made under the original key; and what must be refused: a flipped byte, swapped powers,
another tau's opening key, P_0 != g, a power outside the subgroup (named by index and status), bad lengths."""
import os
import sys

import pytest
import torch

import plonk_gadgets_amd as pg

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import g1_codec_model as M  # noqa: E402
import g1_model as G  # noqa: E402

R = G.R_FR
TAU = 0x5EED_7A0 ** 9 % R
S = pg.BlsScalar.from_int


@pytest.fixture(scope="module")
def engine():
    e = pg.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def key_2_20(engine):
    return pg.CommitKey.setup(engine, (1 << 20) - 1, S(TAU))


def test_to_bytes_is_the_models_encoding_of_the_powers(engine, key_2_20):
    data = key_2_20.trim(63).to_bytes()
    want, t = [], 1
    for _ in range(64):
        want.append(G.compressed(G.mul(t, G.G)))
        t = t * TAU % R
    assert data == b"".join(want)
    assert data[:48] == M.GENERATOR_COMPRESSED


@pytest.mark.parametrize("n", [1, 2, (1 << 10) + 3, 1 << 20])
def test_from_bytes_inverts_to_bytes(engine, key_2_20, n):
    key = key_2_20.trim(n - 1)
    data = key.to_bytes()
    assert len(data) == 48 * n
    back = pg.CommitKey.from_bytes(engine, data)
    assert back.max_degree == n - 1 and torch.equal(back.powers, key.powers)
    if n <= 2048:
        assert torch.equal(pg.CommitKey.from_bytes(engine, data, check=False).powers, key.powers)


def test_save_and_load_with_a_chunk_boundary_and_a_prefix(engine, key_2_20, tmp_path):
    key = key_2_20.trim(2999)
    path = str(tmp_path / "ck.bin")
    key.save(path, chunk=1000)
    assert open(path, "rb").read() == key.to_bytes()
    for chunk in (1024, 1000, 3000, 1 << 20, 1):
        if chunk == 1:
            back = pg.CommitKey.load(engine, path, max_degree=6, chunk=1)
            assert torch.equal(back.powers, key.powers[:7])
            continue
        assert torch.equal(pg.CommitKey.load(engine, path, chunk=chunk).powers, key.powers)
    pre = pg.CommitKey.load(engine, path, max_degree=1499, chunk=1024)
    assert pre.max_degree == 1499 and torch.equal(pre.powers, key.powers[:1500])
    with pytest.raises(pg.PolynomialDegreeTooLarge):
        pg.CommitKey.load(engine, path, max_degree=3000)
    # a prefix is read without looking at the rest: a file that is damaged further on still gives it
    raw = bytearray(open(path, "rb").read())
    raw[48 * 2000] &= 0x7F
    open(path, "wb").write(bytes(raw))
    assert torch.equal(pg.CommitKey.load(engine, path, max_degree=1499, chunk=512).powers, key.powers[:1500])
    with pytest.raises(ValueError, match="power 2000 .*PG_G1_BAD_ENCODING"):
        pg.CommitKey.load(engine, path, chunk=512)


def test_bad_lengths_and_bad_points_are_refused_by_name(engine, key_2_20, tmp_path):
    data = key_2_20.trim(99).to_bytes()
    with pytest.raises(ValueError, match="multiple of 48"):
        pg.CommitKey.from_bytes(engine, data[:-1])
    with pytest.raises(ValueError, match="empty"):
        pg.CommitKey.from_bytes(engine, b"")
    path = str(tmp_path / "short.bin")
    open(path, "wb").write(data[:100])
    with pytest.raises(ValueError, match="multiple of 48"):
        pg.CommitKey.load(engine, path)
    open(path, "wb").write(b"")
    with pytest.raises(ValueError, match="empty"):
        pg.CommitKey.load(engine, path)
    # a power replaced by a curve point outside the subgroup
    import random
    off = G.compressed(M.curve_point_from_x(random.Random(8)))
    bad = data[:48 * 41] + off + data[48 * 42:]
    with pytest.raises(ValueError, match="power 41 .*PG_G1_NOT_IN_SUBGROUP"):
        pg.CommitKey.from_bytes(engine, bad)
    # ... which check=False lets through, as the point it is
    loose = pg.CommitKey.from_bytes(engine, bad, check=False)
    assert loose.powers[41].cpu().tolist() != key_2_20.powers[41].cpu().tolist()
    assert engine.g1_check(loose.powers).cpu().tolist() == [0] * 41 + [M.NOT_IN_SUBGROUP] + [0] * 58
    # an x with no point
    x = 1
    while pow(x * x * x + 4, (M.P - 1) // 2, M.P) == 1:
        x += 1
    with pytest.raises(ValueError, match="power 99 .*PG_G1_NOT_ON_CURVE"):
        pg.CommitKey.from_bytes(engine, data[:48 * 99] + M.raw_x(x, 0x80))


def test_prove_and_verify_under_loaded_parameters(engine, tmp_path):
    """parameters saved with one tau, loaded by an object that never sees it, trimmed; the proof made under the loaded commit key
    verifies under the loaded opening key and is byte for byte the proof made under the original key"""
    pp = pg.PublicParameters.setup(engine, 1 << 12, S(TAU))
    assert pp.is_consistent()
    path = str(tmp_path / "pp.bin")
    pp.save(path)
    assert os.path.getsize(path) == 240 + 48 * ((1 << 12) + 1)
    assert open(path, "rb").read() == pp.to_bytes()
    loaded = pg.PublicParameters.load(engine, path, chunk=1500)
    assert loaded.max_degree == 1 << 12 and torch.equal(loaded.commit_key.powers, pp.commit_key.powers)
    with pytest.raises(pg.PolynomialDegreeTooLarge):
        loaded.trim((1 << 12) + 1)
    ck, ok = loaded.trim(1 << 10)
    assert ck.max_degree == 1 << 10

    def circuit():
        comp = pg.StandardComposer(engine, 1 << 12, 1 << 12)
        res = pg.range_check(comp, S(50_000), S(250_000), pg.AllocatedScalar.allocate(comp, S(70_000)))
        comp.constrain_to_constant(res, S(1), None)
        comp.sync()
        return comp
    comp = circuit()
    assert comp.check() == -1
    proof = comp.prove(ck, b"testing")
    vk = comp.verifier_key(ck)
    assert proof.verify(vk, ok, {}, b"testing")
    assert not proof.verify(vk, ok, {}, b"plonk")
    comp.close()
    comp = circuit()
    original = comp.prove(pp.commit_key.trim(1 << 10), b"testing")
    comp.close()
    assert proof.to_bytes() == original.to_bytes()
    # a prefix of the file is enough for this circuit
    small = pg.PublicParameters.load(engine, path, max_degree=1 << 10)
    assert small.max_degree == 1 << 10 and small.is_consistent()
    assert pg.PublicParameters.from_bytes(engine, pp.to_bytes()).to_bytes() == pp.to_bytes()
    for p in (pp, loaded, small):
        p.opening_key.close()


def test_inconsistent_parameters_are_refused(engine, tmp_path):
    n = 600
    pp = pg.PublicParameters.setup(engine, n - 1, S(TAU))
    data = pp.to_bytes()
    path = str(tmp_path / "pp.bin")
    # one byte flipped in a power: it no longer decodes to a member of G1 (or to anything)
    raw = bytearray(data)
    raw[240 + 48 * 123 + 20] ^= 0x10
    open(path, "wb").write(bytes(raw))
    with pytest.raises(ValueError, match="power 123 "):
        pg.PublicParameters.load(engine, path)
    with pytest.raises(ValueError, match="power 123 "):
        pg.PublicParameters.from_bytes(engine, bytes(raw))
    # two powers swapped: every point is in G1, the key is not a key
    raw = bytearray(data)
    a, b = 240 + 48 * 17, 240 + 48 * 400
    raw[a:a + 48], raw[b:b + 48] = data[b:b + 48], data[a:a + 48]
    open(path, "wb").write(bytes(raw))
    with pytest.raises(ValueError, match="successive powers"):
        pg.PublicParameters.load(engine, path)
    swapped = pg.PublicParameters.load(engine, path, check=False)
    assert swapped.is_consistent() is False
    assert not engine.g1_check(swapped.commit_key.powers).any().item()
    swapped.opening_key.close()
    # the last power alone replaced by another member of G1
    raw = bytearray(data)
    raw[-48:] = data[240 + 48:240 + 96]
    with pytest.raises(ValueError, match="successive powers"):
        pg.PublicParameters.from_bytes(engine, bytes(raw))
    # powers of tau with the opening key of another tau
    other = pg.OpeningKey.setup(engine, S(TAU + 1))
    assert pg.PublicParameters(pp.commit_key, other).is_consistent() is False
    with pytest.raises(ValueError, match="successive powers"):
        pg.PublicParameters.from_bytes(engine, other.to_bytes() + data[240:])
    other.close()
    # P_0 != g: the powers of tau over another base are consistent among themselves, not with g
    base = pg.G1Affine.from_ints(*G.mul(5, G.G))
    shifted = pg.CommitKey.setup(engine, n - 1, S(TAU), base)
    assert pg.PublicParameters(shifted, pp.opening_key).is_consistent() is False
    ok5 = pg.OpeningKey.setup(engine, S(TAU), base)
    assert pg.PublicParameters(shifted, ok5).is_consistent() is True
    ok5.close()
    # one power and two powers
    assert pg.PublicParameters(pp.commit_key.trim(0), pp.opening_key).is_consistent()
    assert pg.PublicParameters(pp.commit_key.trim(1), pp.opening_key).is_consistent()
    two = pp.commit_key.powers[:2].clone()
    two[1] = pp.commit_key.powers[2]
    assert pg.PublicParameters(pg.CommitKey(engine, two), pp.opening_key).is_consistent() is False
    with pytest.raises(ValueError, match="opening key"):
        pg.PublicParameters.from_bytes(engine, data[:100])
    pp.opening_key.close()
