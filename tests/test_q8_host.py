"""int8 feature ingest, host side (no GPU): rnnt_quantize_features_host against the CPU restatement's
quantiser (oracle.quantize = oracle_q8: rintf, clamp to [-128, 127]), the dtype dispatch of Engine's
encode calls, and the error paths of the new entry points.

NaN: the device q8 is fminf(fmaxf(rintf(v), -128), 127), and fmaxf(NaN, -128) = -128, so NaN quantises
to -128 on the device; the host quantiser is written to do the same.  oracle_q8 converts the NaN itself
to an integer (undefined in C), so NaN is checked against -128, not against the restatement."""
import ctypes as C

import numpy as np
import pytest
import torch

from rnnt_amd import _lib
from rnnt_amd.engine import Engine

GUARD = 0x5A


def host_q8(x, scale, in_off=0, out_off=0):
    """rnnt_quantize_features_host on a copy of x placed in_off floats into its buffer, written out_off
    bytes into a guarded output buffer; checks the guard bytes on both sides."""
    x = np.asarray(x, np.float32).ravel()
    n = x.size
    src = np.zeros(n + in_off + 1, np.float32)
    src[in_off: in_off + n] = x
    dst = np.full(n + out_off + 2, GUARD, np.int8)
    rc = _lib.lib().rnnt_quantize_features_host(src.ctypes.data + 4 * in_off, n, C.c_float(scale),
                                                dst.ctypes.data + out_off + 1)
    assert rc == _lib.RNNT_OK
    assert np.all(dst[: out_off + 1] == GUARD) and dst[out_off + 1 + n] == GUARD, "guard byte overwritten"
    return dst[out_off + 1: out_off + 1 + n].copy()


@pytest.mark.parametrize("scale", [8.0, 0.5, 23.716, 0.0371])  # two powers of two, two that are not
def test_matches_oracle_on_normals(oracle, scale):
    x = np.random.default_rng(7).standard_normal(100_000).astype(np.float32) * np.float32(60.0 / scale)
    got = host_q8(x, scale)
    want = oracle.quantize(x, scale)
    assert got.min() == -128 and got.max() == 127  # the clamp is exercised on both sides
    np.testing.assert_array_equal(got, want)


def tie_cases():
    """(x, scale) whose product is exactly k + 0.5: every k in [-130, 130] for power-of-two scales, and
    for the scale 1.5 the odd integers x (x * 1.5 = 3j + 1.5)."""
    k = np.arange(-130, 131, dtype=np.float64)
    cases = [(((k + 0.5) / s).astype(np.float32), s) for s in (1.0, 0.5, 4.0)]
    cases.append((np.arange(-89, 90, 2, dtype=np.float32), 1.5))
    for x, s in cases:
        p = x.astype(np.float64) * s
        assert np.all(p - np.floor(p) == 0.5) and np.all((x * np.float32(s)).astype(np.float64) == p)
    return cases


def test_ties_round_to_even(oracle):
    for x, s in tie_cases():
        got = host_q8(x, s)
        np.testing.assert_array_equal(got, oracle.quantize(x, s))
        p = x.astype(np.float64) * s
        even = 2.0 * np.round(p / 2.0)  # the even neighbour of k + 0.5
        np.testing.assert_array_equal(got, np.clip(even, -128, 127).astype(np.int8))


SPECIALS = np.array([0.0, -0.0, 1e-42, -1e-42, 1e30, -1e30, np.inf, -np.inf], np.float32)


def test_specials(oracle):
    for s in (1.0, 23.716):
        got = host_q8(SPECIALS, s)
        np.testing.assert_array_equal(got, [0, 0, 0, 0, 127, -128, 127, -128])
        np.testing.assert_array_equal(got, oracle.quantize(SPECIALS, s))


def test_nan_gives_minus_128():
    x = np.array([np.nan, 1.0, -np.nan, 2.0, np.nan], np.float32)
    np.testing.assert_array_equal(host_q8(x, 3.0), [-128, 3, -128, 6, -128])
    # in the vector body as well as in the scalar tail
    x = np.full(100, np.nan, np.float32)
    assert np.all(host_q8(x, 1.0) == -128)


@pytest.mark.parametrize("n", [0, 1, 3, 239, 240, 241])
def test_lengths_and_unaligned_pointers(oracle, n):
    x = (np.random.default_rng(n).standard_normal(n) * 40).astype(np.float32)
    want = oracle.quantize(x, 2.5) if n else np.zeros(0, np.int8)
    for in_off, out_off in ((0, 0), (1, 1), (1, 0), (0, 1), (3, 2)):
        np.testing.assert_array_equal(host_q8(x, 2.5, in_off, out_off), want)


def test_bad_arguments():
    lib = _lib.lib()
    out = np.zeros(4, np.int8)
    assert lib.rnnt_quantize_features_host(None, 4, C.c_float(1.0), out.ctypes.data) == _lib.RNNT_EINVAL
    assert lib.rnnt_quantize_features_host(out.ctypes.data, -1, C.c_float(1.0), out.ctypes.data) == _lib.RNNT_EINVAL
    assert lib.rnnt_quantize_features_host(None, 0, C.c_float(1.0), None) == _lib.RNNT_OK
    s = C.c_float(0)
    assert lib.rnnt_engine_input_scale(None, C.byref(s)) == _lib.RNNT_EINVAL
    assert b"null" in lib.rnnt_last_error()
    lh = np.zeros(1, np.int32)
    assert lib.rnnt_engine_encode_gather_q8(None, None, None, None, lh.ctypes.data, 1, 1, 256, None,
                                            None) == _lib.RNNT_EINVAL
    assert lib.rnnt_engine_encode_q8(None, None, None, None, 1, 1, 256, None, None) == _lib.RNNT_EINVAL
    assert lib.rnnt_engine_encode_stream_q8(None, None, None, None, lh.ctypes.data, lh.ctypes.data, 1, 1, 256,
                                            None) == _lib.RNNT_EINVAL
    assert lib.rnnt_engine_encode_stream_pl_q8(None, None, None, None, lh.ctypes.data, lh.ctypes.data, 1, 1, 256,
                                               None) == _lib.RNNT_EINVAL


# ---- Engine's dtype dispatch, against a library that records the entry points called
class _RecordingLib:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def entry(*args):
            self.calls.append(name)
            return 0
        return entry


class _Stream:
    cuda_stream = 0


def _engine():
    eng = Engine.__new__(Engine)
    eng._lib, eng._h = _RecordingLib(), C.c_void_p(1)
    return eng


def _calls(eng, dtype):
    store = torch.zeros((8, 240), dtype=dtype)
    feats = torch.zeros((2, 256, 256), dtype=dtype)
    off = torch.zeros(2, dtype=torch.int64)
    lens = torch.zeros(256, dtype=torch.int32)
    reset = torch.zeros(256, dtype=torch.int32)
    lh = np.array([2, 1], np.int32)
    st = _Stream()
    eng.encode(feats, lens, lh, stream=st)
    eng.encode_gather(store, off, lens, lh, 2, 2, 256, stream=st)
    eng.encode_stream(store, off, lens, lh, reset, 2, 2, 256, stream=st)
    eng.encode_stream_pl(store, off, lens, lh, reset, 2, 2, 256, stream=st)
    return eng._lib.calls


def test_engine_dispatches_on_the_feature_dtype():
    base = ["rnnt_engine_encode", "rnnt_engine_encode_gather", "rnnt_engine_encode_stream",
            "rnnt_engine_encode_stream_pl"]
    assert _calls(_engine(), torch.float32) == base
    assert _calls(_engine(), torch.int8) == [b + "_q8" for b in base]
    for dt in (torch.float16, torch.uint8, torch.float64):
        eng = _engine()
        with pytest.raises(TypeError, match="float32 or torch.int8"):
            _calls(eng, dt)
        assert eng._lib.calls == []
