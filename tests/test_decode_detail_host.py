"""Host side of the detail decode (CPU): word timestamps from per-token frames and confidences
(rnnt_amd.timing.word_timings) and the two new C entry points in the header, the bindings and the
built library."""
import numpy as np
import pytest

from rnnt_amd import _lib, timing
from rnnt_amd.config import FRAME_SECONDS, LABELS

NEW = ("rnnt_engine_decode_detail", "rnnt_engine_decode_stream_detail")


def _ids(text):
    return [LABELS.index(ch) for ch in text]


def test_frame_unit_comes_from_the_config_constants():
    assert FRAME_SECONDS == pytest.approx(0.06, abs=1e-15)  # 10 ms hop x splicing 3 x stacking 2


def test_word_timings_plain_row():
    toks = _ids("hi yo")
    frames = [2, 2, 3, 7, 9]
    conf = [0.9, 0.5, 0.99, 0.8, 0.7]
    w = timing.word_timings(toks, frames, conf)
    assert [x[0] for x in w] == ["hi", "yo"]
    assert w[0][1:] == pytest.approx((2 * 0.06, 3 * 0.06, 0.5))
    assert w[1][1:] == pytest.approx((7 * 0.06, 10 * 0.06, 0.7))


def test_word_timings_leading_trailing_and_double_spaces():
    toks = _ids("  a  it's ")
    frames = list(range(len(toks)))
    conf = [1.0 - 0.01 * i for i in range(len(toks))]
    w = timing.word_timings(toks, frames, conf)
    assert [x[0] for x in w] == ["a", "it's"]
    assert w[0][1:] == pytest.approx((2 * 0.06, 3 * 0.06, conf[2]))
    assert w[1][1:] == pytest.approx((5 * 0.06, 9 * 0.06, conf[8]))
    # a word made of one frame's tokens (the joint emits several per frame) is one frame long
    w = timing.word_timings(_ids("abc"), [4, 4, 4], [0.3, 0.2, 0.6])
    assert len(w) == 1 and w[0][0] == "abc" and w[0][1:] == pytest.approx((0.24, 0.30, 0.2))


def test_word_timings_empty_and_spaces_only():
    assert timing.word_timings([], [], []) == []
    assert timing.word_timings(_ids("   "), [0, 1, 1], [0.5, 0.5, 0.5]) == []


def test_word_timings_accepts_arrays_and_refuses_untrimmed_rows():
    w = timing.word_timings(np.array(_ids("ok"), np.int32), np.array([1, 5], np.int32), np.array([0.25, 0.75], np.float32))
    assert len(w) == 1 and w[0][0] == "ok" and w[0][1:] == pytest.approx((0.06, 0.36, 0.25))
    with pytest.raises(ValueError):
        timing.word_timings(_ids("ok"), [1], [0.5, 0.5])
    with pytest.raises(ValueError):
        timing.word_timings([1, -1], [0, 0], [0.5, 0.5])  # the -1 fill past res_len


def test_new_symbols_are_declared_bound_and_exported():
    names = _lib.header_functions()
    for n in NEW:
        assert n in names, f"{n} not declared in include/rnnt_mi355x.h"
        assert n in _lib._SIGS, f"{n} not bound in rnnt_amd/_lib.py"
    # the plain signatures plus emit_frame and emit_conf
    assert len(_lib._SIGS[NEW[0]][1]) == len(_lib._SIGS["rnnt_engine_decode"][1]) + 2
    assert len(_lib._SIGS[NEW[1]][1]) == len(_lib._SIGS["rnnt_engine_decode_stream"][1]) + 2
    lib = _lib.lib()
    for n in NEW:
        assert hasattr(lib, n), f"librnnt_mi355x.so does not export {n}"
    assert lib.rnnt_abi_version() == 8  # additive: the ABI version stays
    # the argument checks of the plain calls apply (no engine: refused before anything runs)
    assert lib.rnnt_engine_decode_detail(None, None, None, 1, None, None, None) == _lib.RNNT_EINVAL
    assert lib.rnnt_engine_decode_stream_detail(None, None, None, 1, None, None, None, None) == _lib.RNNT_EINVAL
