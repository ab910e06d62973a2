"""PublicParameters: a commit key and an opening key that belong together (dusk-plonk's PublicParameters), made with a known tau
for development or loaded from bytes -- in which case nobody here knows tau, and is_consistent() is what ties the two halves.

Bytes: the 240 bytes of OpeningKey.to_bytes() followed by the commit key's 48 bytes per power.  That is dusk-plonk 0.8's
PublicParameters::to_var_bytes as recalled [DEP-RECALL]: the container's parity is unpinned, like the transcript labels; the
point encodings are the standard ones and are pinned by the tests."""
from __future__ import annotations

import os

import numpy as np
import torch

from .g1 import LOAD_CHUNK, CommitKey, G1Affine, PolynomialDegreeTooLarge, P, points_tensor
from .g2 import OpeningKey

# scalars drawn per pass of is_consistent (32 bytes each on the device)
_RHO_CHUNK = 1 << 22


class PublicParameters:
    def __init__(self, commit_key: CommitKey, opening_key: OpeningKey):
        if commit_key.engine is not opening_key.engine:
            raise ValueError("the two keys live on different engines")
        self.commit_key, self.opening_key = commit_key, opening_key
        self.engine = commit_key.engine

    @staticmethod
    def setup(engine, max_degree: int, tau) -> "PublicParameters":
        """an INSECURE development SRS: whoever knows tau can forge proofs (CommitKey.setup, OpeningKey.setup)"""
        return PublicParameters(CommitKey.setup(engine, max_degree, tau), OpeningKey.setup(engine, tau))

    @property
    def max_degree(self) -> int:
        return self.commit_key.max_degree

    def trim(self, degree: int):
        """(CommitKey, OpeningKey) for polynomials of degree <= `degree`; PolynomialDegreeTooLarge beyond the key"""
        return self.commit_key.trim(degree), self.opening_key

    # ---- bytes ---------------------------------------------------------------------------------------------------------------
    def to_bytes(self) -> bytes:
        return self.opening_key.to_bytes() + self.commit_key.to_bytes()

    def save(self, path) -> None:
        with open(path, "wb") as f:
            f.write(self.opening_key.to_bytes())
            for part in self.commit_key._chunks(LOAD_CHUNK):
                f.write(part)

    @staticmethod
    def _checked(pp: "PublicParameters", check: bool) -> "PublicParameters":
        if check and not pp.is_consistent():
            pp.opening_key.close()
            raise ValueError("the commit key's powers are not the successive powers of the opening key's tau")
        return pp

    @staticmethod
    def from_bytes(engine, data: bytes, check: bool = True) -> "PublicParameters":
        """ValueError on a bad length, a bad point (named by index and status) and, with `check`, on a commit key that is not
        consistent with the opening key.  check=False skips the membership tests and the consistency test alike."""
        view = memoryview(data).cast("B")
        if len(view) < OpeningKey.SIZE:
            raise ValueError(f"public parameters start with the {OpeningKey.SIZE} bytes of an opening key")
        ok = OpeningKey.from_bytes(engine, bytes(view[:OpeningKey.SIZE]))
        try:
            ck = CommitKey.from_bytes(engine, view[OpeningKey.SIZE:], check)  # (a view: the powers are not copied here)
        except Exception:
            ok.close()
            raise
        return PublicParameters._checked(PublicParameters(ck, ok), check)

    @staticmethod
    def load(engine, path, max_degree: int | None = None, check: bool = True, chunk: int = LOAD_CHUNK) -> "PublicParameters":
        """from_bytes for a file; the commit key streams as in CommitKey.load, with max_degree only its prefix"""
        with open(path, "rb") as f:
            head = f.read(OpeningKey.SIZE)
        if len(head) < OpeningKey.SIZE:
            raise ValueError(f"public parameters start with the {OpeningKey.SIZE} bytes of an opening key")
        ok = OpeningKey.from_bytes(engine, head)
        try:
            ck = CommitKey.load(engine, path, max_degree, check, chunk, offset=OpeningKey.SIZE)
        except Exception:
            ok.close()
            raise
        return PublicParameters._checked(PublicParameters(ck, ok), check)

    # ---- the two halves belong together ----------------------------------------------------------------------------------------
    def _random_scalars(self, count: int) -> torch.Tensor:
        """`count` scalars below 2^128 from the OS, Montgomery form, int64[count, 4] on the device"""
        out = torch.empty((count, 4), dtype=torch.int64, device=self.engine.device)
        for start in range(0, count, _RHO_CHUNK):
            m = min(_RHO_CHUNK, count - start)
            raw = np.zeros((m, 4), dtype=np.uint64)
            raw[:, :2] = np.frombuffer(os.urandom(16 * m), dtype=np.uint64).reshape(m, 2)
            mont, _, bad = self.engine.scalars_from_canonical(torch.from_numpy(raw.view(np.int64)).to(self.engine.device))
            assert bad == 0  # (below 2^128: always reduced)
            out[start:start + m] = mont
        return out

    def is_consistent(self) -> bool:
        """True iff P_0 == g and P_{i+1} = tau P_i for every power, tau being the opening key's: with 128-bit rho_i drawn from
        the OS AFTER the key is fixed, e(sum rho_i P_{i+1}, h) e(-sum rho_i P_i, [tau]_2) = 1.  If some P_{i+1} != tau P_i, the
        left side is a non-constant polynomial of degree 1 in that rho_i over GT (prime order r), so the test passes with
        probability at most 2^-128.  Two Engine.msm calls over shifted views of the powers and one pg_pairing_check.  The
        points are expected to be in G1 (CommitKey.from_bytes / load with check=True saw to that)."""
        from .verifier import pairing_check
        powers, ok = self.commit_key.powers, self.opening_key
        if G1Affine(powers[0].cpu().tolist()) != ok.g:
            return False
        n = powers.shape[0]
        if n == 1:
            return True
        rho = self._random_scalars(n - 1)
        hi = self.engine.msm(powers[1:], rho)[0]
        lo = self.engine.msm(powers[:-1], rho)[0]
        q = lo.to_ints()
        neg_lo = lo if q is None else G1Affine.from_ints(q[0], (P - q[1]) % P)
        pts = points_tensor([hi, neg_lo], self.engine.device).view(1, 2, 12)
        return bool(pairing_check(self.engine, pts, [ok.prepared_h, ok.prepared_tau_h])[0].item())


__all__ = ["PublicParameters", "PolynomialDegreeTooLarge"]
