"""lvllm_tiled_gemm (csrc/dense_tiled_gemm.hip) through the C ABI, host side only: outside its envelope the entry
returns 3 before any launch and names the argument; the row-range knobs round-trip and ship shut."""
import ctypes

import pytest


@pytest.fixture(scope="module")
def lib():
    from light_vllm_amd import _native
    lib = _native.load_hip_library()
    for f in (lib.lvllm_tiled_gemm, lib.lvllm_set_tuning, lib.lvllm_get_tuning):
        f.restype = ctypes.c_int
    lib.lvllm_last_error.restype = ctypes.c_char_p
    return lib


@pytest.mark.parametrize("N,K,dtype,act,names", [(32, 48, 2, 0, b"K"), (24, 32, 2, 0, b"N"), (48, 32, 1, 2, b"N"),
                                                 (32, 32, 0, 0, b"dtype")])
def test_outside_the_envelope_returns_3_and_names_the_argument(lib, N, K, dtype, act, names):
    rc = lib.lvllm_tiled_gemm(None, None, None, None, 8, N, K, ctypes.c_int64(K), ctypes.c_int64(N), dtype, act, None,
                              ctypes.c_int64(0), None)
    assert rc == 3
    msg = lib.lvllm_last_error()
    assert msg.startswith(b"lvllm_tiled_gemm: " + names + b" "), msg


def test_row_range_knobs_round_trip_and_ship_shut(lib):
    def get(key):
        v = ctypes.c_int(-12345)
        assert lib.lvllm_get_tuning(key, ctypes.byref(v)) == 0, lib.lvllm_last_error()
        return v.value

    lo, hi = get(b"dense_tiled_min_rows"), get(b"dense_tiled_max_rows")
    assert lo > hi  # as shipped no row count takes the tiled route
    try:
        assert lib.lvllm_set_tuning(b"dense_tiled_min_rows", 65) == 0
        assert lib.lvllm_set_tuning(b"dense_tiled_max_rows", 4096) == 0
        assert (get(b"dense_tiled_min_rows"), get(b"dense_tiled_max_rows")) == (65, 4096)
        assert lib.lvllm_set_tuning(b"dense_tiled_min_rows", 0) != 0
        assert lib.lvllm_set_tuning(b"dense_tiled_max_rows", -1) != 0
    finally:
        lib.lvllm_set_tuning(b"dense_tiled_min_rows", lo)
        lib.lvllm_set_tuning(b"dense_tiled_max_rows", hi)
