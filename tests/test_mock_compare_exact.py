"""CPU tier: int64 and datetime64[ns] columns compare exactly with integer and
Timestamp operands.  The composition layer used to turn the operand into a
float before lib.compare_scalar saw it; above 2^53 that merges neighbours
(one double ulp is 256 ns at present-day timestamps), and neither the mock nor
the kernel could undo it.  These run modin_amd/core/dataframe.py over
tests/mocklib.py against pandas."""

import numpy as np
import pytest

from tests import compare_cases as cc
from tests import mocklib


@pytest.fixture()
def mlib(monkeypatch):
    mocklib.install(monkeypatch)
    import modin_amd.pandas as mpd
    yield mpd


@pytest.mark.parametrize("with_nat", [False, True], ids=["plain", "nat"])
def test_mock_datetime_compare_is_exact(mlib, with_nat):
    cc.check_frame_compares(mlib, lambda: cc.datetime_frame(with_nat), "t",
                            list(cc.datetime_operands()))


def test_mock_bigint_compare_is_exact(mlib):
    cc.check_frame_compares(mlib, cc.bigint_frame, "a",
                            [(repr(s), s) for s in cc.BIGINT_OPERANDS])


def test_mock_int_column_float_operand_promotes(mlib):
    """Against a float operand pandas itself compares in float64: 2^53 + 1
    equals float(2^53).  That path keeps its behaviour."""
    pdf = cc.bigint_frame()
    df = mlib.DataFrame(pdf)
    for s in (float(2**53), 2.5):
        for sym, op in cc.OPS.items():
            got = op(df["a"], s).to_pandas().to_numpy().astype(bool)
            np.testing.assert_array_equal(got, op(pdf["a"], s).to_numpy(),
                                          err_msg=f"{sym} {s}")
