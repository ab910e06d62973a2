"""TEST INFRASTRUCTURE: tests/widget_programs.py's Both -- one call on the device composer and on the C oracle's -- with is_less_equal
 among its calls, replayed on the oracle by tests/compare_gate_oracle.py.  dev = None runs the oracle side alone."""
from tests import compare_gate_oracle as co
from tests.widget_programs import Both


class CompareBoth(Both):
    def __init__(self, dev, ora=None):
        super().__init__(dev, ora)
        self.wid = co.CompareWidgets()

    def is_less_equal_each(self, xs, ys, num_bits, strict=False):
        """-> the result Variables"""
        n0 = self.ora.n
        r = self.dev.is_less_equal_each(self.tv(xs), self.tv(ys), num_bits, strict) if self.dev is not None else None
        o = self._same_vars(r, self.wid.is_less_equal_each(self.ora, xs, ys, num_bits, strict))
        self._logged("is_less_equal_each", len(xs), num_bits, n0)
        return o

    def is_less_equal(self, x, y, num_bits, strict=False):
        n0 = self.ora.n
        _, o = self.wid.is_less_equal(self.ora, x, y, num_bits, strict)
        if self.dev is not None:
            assert self.dev.is_less_equal(int(x), int(y), num_bits, strict) == o
        self._logged("is_less_equal", 1, num_bits, n0)
        return o
