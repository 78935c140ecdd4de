"""The row forms (csrc/hrx_rows.hpp: what a reader of witness rows is told, and where a cell of string b lies) as a program of its own under the sanitizers.
No device."""
import os
import subprocess

import numpy as np
import pytest

import halo2_regex_amd as hra
from oracle_lib import ROOT


def test_host_gathers_across_the_block_border_and_their_shape_limits():
    """hrx_rows_of_string_position_major / _planes (interleaved, three planes, the two row stripes of one def) on a second block of 300 strings, 19 rows
    (5 quads: stripes of 3 and 2 slots, 3 octets), against the library-independent inverse planes_to_string_major / position_major_to_string_major; and the
    shapes a reader of rows holds in 32 bits: B above 2^32 - 65 or M above 2^24 is HRX_ERR_ARG before anything is read (csrc/hrx_rows.hpp RowsIn)"""
    B, M = hra.PM_BLOCK + 300, 19
    q4, q8 = 5, 3
    rng = np.random.default_rng(7)
    msk_pm = rng.integers(0, 2 ** 16, size=q8 * 8 * B, dtype=np.uint16)
    picks = [0, 1, hra.PM_BLOCK - 1, hra.PM_BLOCK, B - 1]
    for D, n_bufs, slots in ((3, 3, q4), (1, 2, 3)):
        planes = [rng.integers(0, 2 ** 32, size=slots * 4 * B, dtype=np.uint32) for _ in range(n_bufs)]
        want_r, want_m = hra.planes_to_string_major(planes, msk_pm, B, M, D=D)
        for b in picks:
            r, m = hra.rows_of_string_planes(planes, msk_pm, B, M, b, D=D)
            assert np.array_equal(r, want_r[b]) and np.array_equal(m, want_m[b]), (D, b)
    rec_pm = rng.integers(0, 2 ** 32, size=q4 * 4 * 2 * B, dtype=np.uint32)
    want_r, want_m = hra.position_major_to_string_major(rec_pm, msk_pm, B, M, 2)
    for b in picks:
        r, m = hra.rows_of_string_position_major(rec_pm, msk_pm, B, M, 2, b)
        assert np.array_equal(r, want_r[b]) and np.array_equal(m, want_m[b]), b
    # the limits: refused on the shape alone (one-element buffers: nothing may be read)
    one32, one16, lens = np.zeros(1, np.uint32), np.zeros(1, np.uint16), np.zeros(1, np.uint32)
    for Bx, Mx in ((2 ** 32 - 64, 4), (4, 2 ** 24 + 1)):
        with pytest.raises(hra.HrxError) as e:
            hra.rows_of_string_position_major(one32, one16, Bx, Mx, 1, 0, out=(one32, one16))
        assert e.value.code == hra.HRX_ERR_ARG
        with pytest.raises(hra.HrxError) as e:
            hra.rows_of_string_planes([one32], one16, Bx, Mx, 0, out=(one32, one16))
        assert e.value.code == hra.HRX_ERR_ARG
        cols = np.zeros(8, np.uint64)
        assert hra.lib.hrx_witness_columns_host(0, one16.ctypes.data, 16, lens.ctypes.data, one32.ctypes.data, 0, one16.ctypes.data, 0, Bx, Mx, 1, 0, 1,
                                                cols.ctypes.data) == hra.HRX_ERR_ARG


def test_standalone_program_under_the_sanitizers(tmp_path):
    """tests/host_cpp/test_rows_host.cpp: csrc/hrx_rows.hpp compiled into a program of its own with the address and undefined-behaviour sanitizers — every
    row form built index by index from the formulas of include/hrx.h in heap blocks of exact size, read back through the shared place on both sides of the
    block border, with and without masked rows"""
    exe = str(tmp_path / "hrx_test_rows_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "host_cpp", "test_rows_host.cpp"), "-o", exe, "-pthread"])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "rows host: ok" in out.stdout, out.stdout + out.stderr
