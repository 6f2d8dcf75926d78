"""The featurizer's int8 entries (rnnt_featurizer_run_q8 / _run_rows_q8: plan, logmel into the fp32
scratch, fz_norm_q8_kernel) executed on the CPU by the host emulation of the wave model
(tools/emu/fz_emu.cpp, an AddressSanitizer build, so every access past an exact-size buffer is
caught).  The int8 output must be, byte for byte, the engine's input quantiser
clip(rint(x * s), -128, 127) applied to the emulator's own fp32 output of the same batch -- the
statistics, the normalisation and the quantiser are the same operations in the same order, so there
is no tolerance.  Padding is zero bytes and every byte of the padded form is written (the buffer
starts as 0xA5), the lengths equal the fp32 run's, two LDS poisons give the same bytes (no LDS word
read before it is written), and the rows form writes each sample's frames at its row offset and
leaves every other byte of the store alone."""
import os
import subprocess

import numpy as np
import pytest

from rnnt_amd import synthetic
from rnnt_amd.featurizer import make_window, mel_filterbank

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"

LENS = [0, 1, 479, 480, 3200, 16037, 777]
N, N_PAD = 7, 8
FRAMES = [(1 + v // 160 + 2) // 3 if v > 0 else 0 for v in LENS]  # rnnt_featurizer_frames
T_OUT = max(FRAMES) + 2
SCALES = (16.0, 50.0)


def _run(exe, inp, out, poison, *extra):
    env = dict(os.environ, EMU_POISON=poison, ASAN_OPTIONS="detect_leaks=0")
    r = subprocess.run([exe, inp, out, *extra], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, f"fz_emu {extra} ({poison}) rc={r.returncode}:\n{r.stderr[-3000:]}"
    return np.fromfile(out, np.uint8)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """Every emulator run the tests below look at, made once: the fp32 output, the padded int8
    output per scale (two poisons at the first scale) and the rows form at the first scale."""
    if not os.path.exists(CLANG):
        pytest.skip("no ROCm clang++")
    out = tmp_path_factory.mktemp("emu_fz_q8")
    env = dict(os.environ, EMU_ASAN="1", EMU_OUT=str(out))
    subprocess.run(["bash", os.path.join(REPO, "tools", "emu", "build_fz.sh")], check=True, env=env,
                   capture_output=True, timeout=600)
    exe = str(out / "fz_emu")
    wavs = [np.asarray(w, np.float32) for w in synthetic.make_wavs(LENS, seed=3)]
    wav = np.zeros((N, max(LENS)), np.float32)
    for i, w in enumerate(wavs):
        wav[i, : len(w)] = w
    inp = str(out / "in.bin")
    with open(inp, "wb") as f:
        np.array([N, N_PAD, T_OUT], np.int32).tofile(f)
        np.asarray(make_window("hann", 320), np.float32).tofile(f)
        np.asarray(mel_filterbank(16000, 512, 80), np.float32).tofile(f)
        np.array(LENS, np.int32).tofile(f)
        wav.tofile(f)
    r = {"f32": _run(exe, inp, str(out / "f32.out"), "nan")}
    for s in SCALES:
        r[("q8", s, "nan")] = _run(exe, inp, str(out / f"q8_{s}_nan.out"), "nan", repr(s))
    r[("q8", SCALES[0], "rand")] = _run(exe, inp, str(out / "q8_rand.out"), "rand", repr(SCALES[0]))
    r["rows"] = _run(exe, inp, str(out / "rows.out"), "nan", repr(SCALES[0]), "rows")
    return r


def _split(raw, dtype):
    return raw[: 4 * N_PAD].view(np.int32), raw[4 * N_PAD:].view(dtype).reshape(T_OUT, N_PAD, 256)


@pytest.mark.parametrize("s", SCALES)
def test_q8_bytes_are_the_quantised_fp32_output(runs, s):
    fl, x = _split(runs["f32"], np.float32)
    ql, q = _split(runs[("q8", s, "nan")], np.int8)
    assert fl.tolist() == FRAMES + [0] * (N_PAD - N)
    np.testing.assert_array_equal(ql, fl)
    want = np.clip(np.rint(x * np.float32(s)), -128, 127).astype(np.int8)
    np.testing.assert_array_equal(q, want)
    if s == 50.0:  # the clamp is exercised, on both sides or at least one
        assert np.any((want == 127) | (want == -128))


def test_q8_padding_is_zero_and_every_byte_written(runs):
    _, q = _split(runs[("q8", SCALES[0], "nan")], np.int8)
    # the sentinel byte 0xA5 = -91 as a real value would need v ~ -5.7 at scale 16: the very bound
    # (T - 1) / sqrt(T) of a normalised feature over <= 34 frames, which no log-mel channel comes near
    assert not np.any(q.view(np.uint8) == 0xA5)
    assert not q[:, N:].any() and not q[:, :, 240:].any()
    for i, T in enumerate(FRAMES):
        assert not q[T:, i].any()
        assert T <= 1 or q[:T, i, :240].any()  # one frame is its own mean: all zeros


def test_q8_lds_poisons_agree(runs):
    np.testing.assert_array_equal(runs[("q8", SCALES[0], "nan")], runs[("q8", SCALES[0], "rand")])


def test_q8_rows_form(runs):
    _, q = _split(runs[("q8", SCALES[0], "nan")], np.int8)
    raw = runs["rows"]
    fl = raw[: 4 * N].view(np.int32)
    roff = raw[4 * N: 12 * N].view(np.int64)
    rows = int(raw[12 * N: 12 * N + 8].view(np.int64)[0])
    store = raw[12 * N + 8:].reshape(rows, 240)
    assert fl.tolist() == FRAMES
    assert np.any(np.diff(roff) < 0)  # out of order
    used = np.zeros(rows, bool)
    for i, (r, T) in enumerate(zip(roff, FRAMES)):
        assert not used[r:r + T].any()
        np.testing.assert_array_equal(store[r:r + T].view(np.int8), q[:T, i, :240], err_msg=f"row {i}")
        used[r:r + T] = True
    assert used.sum() == sum(FRAMES) and (~used).sum() > 0  # gaps between the rows
    assert np.all(store[~used] == 0xA5)
