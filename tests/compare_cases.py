"""Frame-level compare cases above 2^53, shared by the mock tier
(test_mock_compare_exact.py) and the GPU tier
(test_gpu_elementwise_edges.py): an int64 or datetime64[ns] column against an
integer or Timestamp operand must compare as pandas does, exactly, and not via
float64, where neighbours within one ulp (256 ns at today's timestamps) merge.
"""

import operator

import numpy as np
import pandas

T0 = pandas.Timestamp("2024-03-01 12:00").value
OPS = {"==": operator.eq, "!=": operator.ne, "<": operator.lt,
       "<=": operator.le, ">": operator.gt, ">=": operator.ge}
# the rows of the issue, then their mirror below t0 and a few far values
OFFSETS = [-1, 0, 1, 100, 255, -100, -255, 2, 256, -256, 10**12, -10**12]


def datetime_frame(with_nat):
    ns = np.array([T0 + d for d in OFFSETS], dtype=np.int64)
    t = pandas.Series(ns.view("datetime64[ns]"), name="t")
    if with_nat:
        t[[3, 7, len(t) - 1]] = pandas.NaT
    return pandas.DataFrame({"t": t})


def datetime_operands():
    yield "Timestamp", pandas.Timestamp(T0 + 1)
    yield "datetime64", np.datetime64(T0 + 1, "ns")


def bigint_frame():
    c = 2**53 + 1
    a = np.array([c + d for d in (-2, -1, 0, 1, 2, 3, -(2**53), 2**9)]
                 + [2**62, 2**62 + 1, 2**62 + 2, -(2**53) - 1, -(2**53)],
                 dtype=np.int64)
    return pandas.DataFrame({"a": a})


BIGINT_OPERANDS = [2**53, 2**53 + 1, 2**53 + 2, 2**62 + 1, -(2**53) - 1,
                   np.int64(2**53 + 1)]


def check_frame_compares(mpd, make_frame, column, operands):
    """Every operator of OPS on mpd's frame against the same on pandas."""
    pdf = make_frame()
    df = mpd.DataFrame(pdf)
    for tag, operand in operands:
        for sym, op in OPS.items():
            got = op(df[column], operand).to_pandas().to_numpy()
            exp = op(pdf[column], operand).to_numpy()
            np.testing.assert_array_equal(
                got.astype(bool), exp, err_msg=f"{column} {sym} {tag}")
