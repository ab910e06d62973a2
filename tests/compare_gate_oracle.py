"""TEST INFRASTRUCTURE, CPU: is_less_equal replayed call for call on the C oracle's composer, which does not
have it: tests/widget_oracle.py's Widgets with one more append.  The layout is that of tests/compare_gate_model.py -- item() says
which Variable sits on which wire and what the k new Variables hold; this module only records that through Widgets._record.

An item is its k new Variables first (k - 1 accumulators of z, then z), then its g + 1 rows; a batch is a loop in item order."""
from tests import compare_gate_model as cm
from tests import widget_oracle as wo


class CompareWidgets(wo.Widgets):
    def is_less_equal(self, ora, x_var, y_var, num_bits, strict=False):
        """-> (the item's first row, the result Variable)"""
        first_var, zero = ora.num_vars, int(ora.L.composer_zero_var(ora.c))
        rows, sel, qr, new, result = cm.item(int(x_var), int(y_var), self._value(ora, x_var), self._value(ora, y_var), num_bits, strict,
                                             first_var, zero)
        return self._record(ora, rows, sel, qr, new, first_var), result

    def is_less_equal_each(self, ora, x_vars, y_vars, num_bits, strict=False):
        """-> the result Variables"""
        assert len(x_vars) == len(y_vars)
        return [self.is_less_equal(ora, x, y, num_bits, strict)[1] for x, y in zip(x_vars, y_vars)]
