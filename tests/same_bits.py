"""Bit equality of two fp32 matrices with a report that locates a fault.  Not a test module."""
import numpy as np
import pytest


def same_bits(name, got, want):
    """bit equality, and on a failure which rows and elements differ: what a fault is located from"""
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    if len(bad):
        rows = np.unique(bad[:, 0])
        pytest.fail(f"{name}: {len(bad)} elements in {len(rows)} rows differ; rows {rows[:16].tolist()}, "
                    f"elements of the first {bad[bad[:, 0] == rows[0], 1][:16].tolist()}, "
                    f"largest difference {float(np.abs(got - want).max())}", pytrace=False)
