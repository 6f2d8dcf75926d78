"""The featurizer's int8 entries (rnnt_featurizer_run_q8 / _run_rows_q8) on the GPU.

The contract is exact: every byte is q8(v * scale) of the fp32 value the fp32 entry writes at that
position -- the bytes ``engine.quantize`` makes of the fp32 output -- and padding is zero bytes.  The
statistics, the normalisation and the quantiser are the same operations in the same order, so
every comparison here is byte for byte; and since the encoder after the quantiser is integer
arithmetic, Offline and Server answers over int8 WAV input equal the fp32 ones token for token.
"""
import time

import numpy as np
import pytest

from rnnt_amd import synthetic

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

# configs/rnnt.toml [input_eval] (tests/test_featurizer_gpu.py)
INPUT_EVAL = dict(normalize="per_feature", sample_rate=16000, window_size=0.02, window_stride=0.01, window="hann",
                  features=80, n_fft=512, frame_splicing=3, dither=0.00001, feat_type="logfbank", pad_to=0)

LENS = [0, 1, 100, 257, 479, 480, 16037, 160 * 96 + 5, 96000, 239999, 240000]
ROW_LENS = [48000, 3200, 0, 777, 150000, 1]


def _new_featurizer():
    from rnnt_amd.featurizer import AudioProcessing
    return AudioProcessing("quant", **INPUT_EVAL).featurizer


@pytest.fixture(scope="module")
def fz():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    f = _new_featurizer()
    yield f
    f.close()


@pytest.fixture(scope="module")
def pm():
    from rnnt_amd import weights
    return weights.build_model()[0]


@pytest.fixture(scope="module")
def engine(pm):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from rnnt_amd.engine import Engine
    e = Engine(pm, max_batch=256, max_frames=500)
    yield e
    e.close()


@pytest.fixture(scope="module")
def scale(engine):
    return engine.input_scale()


def _batch(wavs):
    n, L = len(wavs), max([len(w) for w in wavs] + [1])
    x = torch.zeros((n, L), dtype=torch.float32)
    for i, w in enumerate(wavs):
        x[i, :len(w)] = w.cpu()
    return x.cuda(), torch.tensor([len(w) for w in wavs], dtype=torch.int32)


def _ragged(wavs):
    L = [len(w) for w in wavs]
    flat = torch.cat([w.cuda() for w in wavs] + [torch.zeros(1, device="cuda")])
    off = torch.tensor(np.concatenate([[0], np.cumsum(L)[:-1]]), dtype=torch.int64, device="cuda")
    return flat, off, torch.tensor(L, dtype=torch.int32)


def _np_q8(x, s):
    return np.clip(np.rint(x * np.float32(s)), -128, 127).astype(np.int8)


def _both(fz, engine, scale, x, lens, n_pad, T_out, **kw):
    """(int8 from the featurizer, its lengths, the fp32 output, engine.quantize of it, fp32 lengths)."""
    q, ql = fz.featurize(x, lens.cuda(), lens.numpy(), n_pad=n_pad, T_out=T_out, scale=scale, **kw)
    f, fl = fz.featurize(x, lens.cuda(), lens.numpy(), n_pad=n_pad, T_out=T_out, **kw)
    want = engine.quantize(f)
    torch.cuda.synchronize()
    assert q.dtype == torch.int8 and tuple(q.shape) == (T_out, n_pad, 256)
    return q.cpu().numpy(), ql.cpu().numpy(), f.cpu().numpy(), want.cpu().numpy(), fl.cpu().numpy()


def test_padded_form_is_the_quantised_fp32_output(fz, engine, scale):
    wavs = synthetic.make_wavs(LENS, seed=21)
    x, lens = _batch(wavs)
    n, n_pad, T_out = len(LENS), 16, 505
    q, ql, f, want, fl = _both(fz, engine, scale, x, lens, n_pad, T_out)
    np.testing.assert_array_equal(ql, fl)
    np.testing.assert_array_equal(q, want)
    np.testing.assert_array_equal(q, _np_q8(f, scale))
    assert q.any()
    # exact zeros in all padding: frames past a row's length, channels 240..255, rows >= n
    assert not q[:, n:].any() and not q[:, :, 240:].any()
    for i in range(n):
        assert not q[fl[i]:, i].any()


def test_rows_form_and_argument_checks(fz, engine, scale):
    from rnnt_amd import _lib
    from rnnt_amd._lib import EngineError
    from rnnt_amd.featurizer import feature_frames
    L = ROW_LENS
    wavs = synthetic.make_wavs(L, seed=26)
    flat, off, lens = _ragged(wavs)
    fr = [feature_frames(v) for v in L]
    a, al = fz.featurize(flat, lens.cuda(), lens.numpy(), n_pad=8, T_out=max(fr), offsets=off, scale=scale)
    store = torch.full((4000, 240), 0x55, dtype=torch.int8, device="cuda")
    rows = np.array([3000, 10, 2000, 400, 1000, 3990], np.int64)  # out of order, gaps between
    fl = fz.featurize_rows(flat, lens.cuda(), lens.numpy(), store, rows, max_frames=max(fr), offsets=off, scale=scale)
    torch.cuda.synchronize()
    assert fl.cpu().tolist()[:len(L)] == fr == al.cpu().tolist()[:len(L)]
    s, g = store.cpu().numpy(), a.cpu().numpy()
    used = np.zeros(len(s), bool)
    for i, (r, T) in enumerate(zip(rows, fr)):
        np.testing.assert_array_equal(s[r:r + T], g[:T, i, :240], err_msg=f"row {i}")
        used[r:r + T] = True
    assert np.all(s[~used] == 0x55)
    before = store.clone()
    with pytest.raises(ValueError, match="outside the store"):
        fz.featurize_rows(flat, lens.cuda(), lens.numpy(), store, rows + 600, max_frames=max(fr), offsets=off,
                          scale=scale)
    with pytest.raises(ValueError, match="max_frames"):
        fz.featurize_rows(flat, lens.cuda(), lens.numpy(), store, rows, max_frames=max(fr) - 1, offsets=off,
                          scale=scale)
    with pytest.raises(ValueError, match="scale"):
        fz.featurize_rows(flat, lens.cuda(), lens.numpy(), store, rows, max_frames=max(fr), offsets=off)
    with pytest.raises(ValueError, match="scale"):  # and a scale with an fp32 store
        fz.featurize_rows(flat, lens.cuda(), lens.numpy(), torch.empty((4000, 240), device="cuda"), rows,
                          max_frames=max(fr), offsets=off, scale=scale)
    # the C entry's own checks (all before any launch)
    lens_d, rows_d = lens.cuda(), torch.from_numpy(rows).cuda()

    def c_rows(store_ptr, s):
        _lib.check(_lib.lib().rnnt_featurizer_run_rows_q8(fz._h, flat.data_ptr(), off.data_ptr(), 0, lens_d.data_ptr(),
                                                          lens.numpy().ctypes.data, len(L), s, store_ptr,
                                                          rows_d.data_ptr(), fl.data_ptr(), max(fr), None),
                   "run_rows_q8")

    with pytest.raises(EngineError, match="aligned"):
        c_rows(store.data_ptr() + 4, scale)
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(EngineError, match="scale"):
            c_rows(store.data_ptr(), bad)
    with pytest.raises(EngineError, match="aligned"):
        _lib.check(_lib.lib().rnnt_featurizer_run_q8(fz._h, flat.data_ptr(), off.data_ptr(), 0, lens_d.data_ptr(),
                                                     lens.numpy().ctypes.data, len(L), 8, scale, a.data_ptr() + 4,
                                                     al.data_ptr(), max(fr), None), "run_q8")
    torch.cuda.synchronize()
    assert torch.equal(store, before)  # a refused call writes nothing


def test_input_form_does_not_matter(fz, scale):
    L = ROW_LENS[:5]
    wavs = synthetic.make_wavs(L, seed=22)
    x, lens = _batch(wavs)
    a, al = fz.featurize(x, lens.cuda(), lens.numpy(), n_pad=8, T_out=320, scale=scale)
    flat, off, _ = _ragged(wavs)
    b, bl = fz.featurize(flat, lens.cuda(), lens.numpy(), n_pad=8, T_out=320, offsets=off, scale=scale)
    # one row alone (same T_out) == the same row inside the batch
    c, _ = fz.featurize(x[4:5].contiguous(), lens[4:5].cuda(), lens[4:5].numpy(), n_pad=1, T_out=320, scale=scale)
    torch.cuda.synchronize()
    assert torch.equal(a, b) and torch.equal(al, bl)
    assert torch.equal(c[:, 0], a[:, 4])
    assert a[:, 4].any()
    with pytest.raises(ValueError, match="int8"):  # a passed out must match
        fz.featurize(x, lens.cuda(), lens.numpy(), n_pad=8, T_out=320, scale=scale,
                     out=torch.empty((320, 8, 256), device="cuda"))


def test_scratch_grows_and_is_reused(engine, scale):
    """One featurizer object: a small batch, a batch that grows the scratch, the small batch again
    (now in a larger scratch, with another row stride than the large batch left behind)."""
    own = _new_featurizer()
    try:
        small = synthetic.make_wavs([3200, 777], seed=27)
        big = synthetic.make_wavs(LENS, seed=21)
        for wavs, n_pad, T_out in ((small, 2, 8), (big, 16, 505), (small, 2, 8)):
            x, lens = _batch(wavs)
            q, ql, _, want, fl = _both(own, engine, scale, x, lens, n_pad, T_out)
            np.testing.assert_array_equal(q, want)
            np.testing.assert_array_equal(ql, fl)
            assert q.any()
    finally:
        own.close()


def test_offline_over_quantized_wav_qsl(engine):
    from rnnt_amd.sut import GpuWavQSL, OfflineSUT, make_batches
    frames = np.minimum(synthetic.devclean_lengths(24, seed=61), 200)
    wavs = synthetic.make_wavs(synthetic.wav_lengths_for_frames(frames, seed=61), seed=61, device="cuda")
    qsl = GpuWavQSL(wavs)
    q8 = qsl.quantized(engine)
    assert q8.store is qsl.store and qsl.q8_scale is None  # a view of the same audio
    x, _, _ = q8.assemble([0, 1, 2])
    assert x.dtype == torch.int8 and qsl.assemble([0, 1, 2])[0].dtype == torch.float32
    ids = np.arange(len(frames))
    got = {}
    for name, q in (("fp32", qsl), ("int8", q8)):
        off = OfflineSUT(engine, q, batch_size=16)
        off.issue_batches(make_batches(q, ids, ids, 16))
        got[name] = off.responses
    assert sum(len(got["fp32"][k]) for k in ids) > 0
    for k in ids:
        np.testing.assert_array_equal(got["int8"][k], got["fp32"][k], err_msg=f"sample {k}")


@pytest.fixture(scope="module")
def server_case(engine):
    """The Server tests' audio, query and the Offline answer over the fp32 QSL (computed once)."""
    from rnnt_amd.sut import GpuWavQSL, OfflineSUT, make_batches
    count, n = 60, 150
    frames = np.minimum(synthetic.devclean_lengths(count, seed=71), 200)
    wavs = synthetic.make_wavs(synthetic.wav_lengths_for_frames(frames, seed=71), seed=71, device="cuda")
    index = np.random.default_rng(72).integers(0, count, size=n)
    qsl = GpuWavQSL(wavs)
    off = OfflineSUT(engine, qsl, batch_size=256)
    off.issue_batches(make_batches(qsl, np.arange(n), index, 256))
    return wavs, index, off.responses


@pytest.mark.parametrize("pipelined", [False, True], ids=["rounds", "pipelined"])
def test_server_over_int8_wav_feeds(pm, scale, server_case, pipelined):
    from rnnt_amd.engine import Engine
    from rnnt_amd.sut import GpuWavQSL, QuerySample, ServerSUT, WavFeed
    wavs, index, offline = server_case
    n = len(index)
    qsls = [GpuWavQSL(wavs) for _ in range(2)]
    engines = [Engine(pm, device=0, max_batch=256, max_frames=500) for _ in range(2)]
    feeds = [WavFeed(q, pro_batch=32, q8_scale=scale) for q in qsls]
    arrivals = np.cumsum(np.random.default_rng(73).exponential(1.0 / 1500.0, size=n))
    try:
        assert all(e.input_scale() == scale for e in engines)
        srv = ServerSUT(engines, slots=256, split_len=32, pipelined=pipelined, feeds=feeds)
        assert all(f.store.feats.dtype == torch.int8 for f in feeds)
        srv.start()
        t0 = time.perf_counter()
        i = 0
        while i < n:
            j = int(np.searchsorted(arrivals, time.perf_counter() - t0, side="right"))
            if j > i:
                for k in range(i, j):
                    srv.issue_query([QuerySample(id=k, index=int(index[k]))], now=t0 + arrivals[k])
                i = j
            else:
                time.sleep(0.0005)
        deadline = time.time() + 60
        while len(srv.latency) < n and time.time() < deadline and not srv.errors:
            time.sleep(0.005)
        srv.stop()
    finally:
        for e in engines:
            e.close()
    assert not srv.errors, srv.errors
    assert len(srv.responses) == n
    for f in feeds:  # both lanes featurized work into int8 stores; every store slot came back
        assert f.batches > 0 and f.store.free == f.store.slots and f.store.feats.dtype == torch.int8
    for k in range(n):
        np.testing.assert_array_equal(srv.responses[k], offline[k], err_msg=f"sample {k} (QSL {index[k]})")
