"""int8 feature ingest on the GPU: features quantised once (rnnt_quantize_features / _host) and encoded
through the _q8 entry points give bit-identical encoder outputs and identical tokens to the fp32 path and
to the CPU restatement -- everything after the input quantiser is int8 -> int32, so every check here is
an equality.  Small shapes: 40 rows in n_pad = 256, T <= 33 (the harness fixture, copied from
tests/test_sut_harness_gpu.py, goes to 61 frames)."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest
import torch

from rnnt_amd import _lib, dist, synthetic, weights
from rnnt_amd._lib import EngineError
from rnnt_amd.engine import Engine
from rnnt_amd.sut import FeatureStore, GpuQSL, OfflineSUT, make_batches

from test_q8_host import SPECIALS, host_q8, tie_cases

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(REPO, "rnnt-inference_amd", "rnnt_amd", "rnnt_sut_harness")
N, NP, T = 40, 256, 33


@pytest.fixture(scope="module")
def pm():
    return weights.build_model()[0]


@pytest.fixture(scope="module")
def eng(pm):
    e = Engine(pm, device=0, max_batch=NP, max_frames=64)
    yield e
    e.close()


@pytest.fixture(scope="module")
def data(pm, oracle):
    """40 utterances (lengths 0, 1, 2, odd ones and T among them), the CPU restatement's encoder output
    and tokens, and a ragged fp32 store that holds them in shuffled order with gaps of other values
    between them: row offsets are arbitrary frame indices (16-byte, not 256-byte aligned, as int8)."""
    rng = np.random.default_rng(93)
    lens = rng.integers(1, T + 1, N).astype(np.int32)
    lens[[0, 1, 2, 4]] = [33, 16, 17, 20]   # the stream test's utterances
    lens[[3, 5, 9, 22, 17]] = [0, 1, 2, 33, 31]
    x = synthetic.make_features(T, N, seed=52, lens=lens)  # [T][N][256]
    fo = oracle.encoder_i8(pm, x, lens)
    ro, rlo, _ = oracle.greedy_decode(pm, fo, (lens + 1) // 2, max_res=32 * 30)
    assert rlo.max() > 3 and rlo[3] == 0 and int(rlo.sum()) > 40
    offsets, rows, at = np.zeros(N, np.int64), [], 0
    for i in rng.permutation(N):
        gap = int(rng.integers(1, 4))
        rows.append(rng.standard_normal((gap, 240)).astype(np.float32) * 50)
        offsets[i] = at + gap
        rows.append(x[: lens[i], i, :240])
        at += gap + int(lens[i])
    rows.append(np.full((2, 240), 99.0, np.float32))
    assert len(set(offsets.tolist())) == N and np.any(offsets % 16 != 0)
    return dict(lens=lens, x=x, fo=fo, want=[ro[i, : rlo[i]] for i in range(N)], offsets=offsets,
                store=torch.from_numpy(np.concatenate(rows)).cuda())


def dev_q8(x, scale):
    """rnnt_quantize_features on the device with any scale."""
    xd = torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda()
    out = torch.empty(xd.shape, dtype=torch.int8, device="cuda")
    rc = _lib.lib().rnnt_quantize_features(xd.data_ptr(), xd.numel(), C.c_float(scale), out.data_ptr(), 0,
                                           C.c_void_p(torch.cuda.current_stream().cuda_stream))
    _lib.check(rc, "rnnt_quantize_features")
    torch.cuda.synchronize()
    return out.cpu().numpy()


def test_device_quantiser_equals_restatement_and_host(eng, pm, oracle):
    s = eng.input_scale()
    assert s == float(np.float32(pm.enc_in_s[0])) and s > 0
    rng = np.random.default_rng(11)
    for n in (100_003, 100_000, 5, 2):  # n % 4 = 3, 0, 1, 2: the float4 body and the tail launch
        x = (rng.standard_normal(n) * (60.0 / s)).astype(np.float32)
        got = eng.quantize(torch.from_numpy(x).cuda()).cpu().numpy()
        np.testing.assert_array_equal(got, oracle.quantize(x, s))
        np.testing.assert_array_equal(got, eng.quantize_host(x))
    for x, sc in tie_cases() + [(SPECIALS, 1.0), (SPECIALS, 23.716)]:
        got = dev_q8(x, sc)
        np.testing.assert_array_equal(got, oracle.quantize(x, sc))
        np.testing.assert_array_equal(got, host_q8(x, sc))
    # NaN: -128 on the device (fmaxf(NaN, -128) = -128) and on the host; the restatement's conversion of a
    # NaN is undefined, so it is not consulted
    x = np.array([np.nan, 1.0, -np.nan, np.nan, 2.0, np.nan, np.nan], np.float32)
    np.testing.assert_array_equal(dev_q8(x, 3.0), [-128, 3, -128, -128, 6, -128, -128])
    np.testing.assert_array_equal(host_q8(x, 3.0), dev_q8(x, 3.0))
    with pytest.raises(TypeError):
        eng.quantize(torch.zeros(8, dtype=torch.float16, device="cuda"))


def _encode_decode(eng, call):
    """call(f_out) enqueues an encode -> (f [Tp][N][1024] host, tokens per row)."""
    f = torch.zeros(((T + 1) // 2, NP, 1024), dtype=torch.float32, device="cuda")
    res = torch.empty((N, eng.max_res), dtype=torch.int32, device="cuda")
    rl = torch.empty(N, dtype=torch.int32, device="cuda")
    call(f)
    eng.decode(res, rl)
    torch.cuda.synchronize()
    rlh, rh = rl.cpu().numpy(), res.cpu().numpy()
    return f.cpu().numpy()[:, :N], [rh[i, : rlh[i]] for i in range(N)]


def _check_against(data, f, toks, f_ref, toks_ref):
    assert np.array_equal(f.view(np.uint32), f_ref.view(np.uint32)), "int8 and fp32 ingest differ in f"
    for i in range(N):
        fl = (data["lens"][i] + 1) // 2
        assert np.array_equal(f[:fl, i].view(np.uint32), data["fo"][:fl, i].view(np.uint32)), f"encoder row {i}"
        np.testing.assert_array_equal(toks[i], toks_ref[i], err_msg=f"row {i} vs fp32 ingest")
        np.testing.assert_array_equal(toks[i], data["want"][i], err_msg=f"row {i} vs restatement")


def _batch(data):
    lp = np.zeros(NP, np.int32)
    lp[:N] = data["lens"]
    return torch.from_numpy(lp).cuda(), torch.from_numpy(data["offsets"]).cuda()


@pytest.mark.parametrize("tile", ["auto", "mini", "big"])
def test_encode_gather_from_int8_store(eng, data, tile):
    lens_d, off_d = _batch(data)
    store, lens = data["store"], data["lens"]
    sq = eng.quantize(store)
    assert sq.dtype == torch.int8 and sq.shape == store.shape and sq.data_ptr() % 16 == 0
    eng.set_tile(tile)
    try:
        f32 = _encode_decode(eng, lambda f: eng.encode_gather(store, off_d, lens_d, lens, T, N, NP, f_out=f))
        q8 = _encode_decode(eng, lambda f: eng.encode_gather(sq, off_d, lens_d, lens, T, N, NP, f_out=f))
    finally:
        eng.set_tile("auto")
    _check_against(data, *q8, *f32)


def test_dense_encode_from_int8_image(eng, data):
    lens_d, _ = _batch(data)
    lens = data["lens"]
    x = np.zeros((T, NP, 256), np.float32)
    x[:, :N] = data["x"]
    xd = torch.from_numpy(x).cuda()
    xq = eng.quantize(xd)
    f32 = _encode_decode(eng, lambda f: eng.encode(xd, lens_d, lens, n=N, f_out=f))
    q8 = _encode_decode(eng, lambda f: eng.encode(xq, lens_d, lens, n=N, f_out=f))
    _check_against(data, *q8, *f32)
    # frames past a row's length, channels 240..255 and padding rows are read as zero whatever they hold,
    # and the engine has its own copy: the caller's buffer may change once the encode's work is done
    junk = xq.clone()
    junk[:, :, 240:] = 77
    junk[:, N:] = -5
    for i in range(N):
        junk[int(lens[i]):, i] = 11

    def call(f):
        eng.encode(junk, lens_d, lens, n=N, f_out=f)
        torch.cuda.synchronize()
        junk.fill_(1)

    _check_against(data, *_encode_decode(eng, call), *f32)


def _stream_tokens(eng, store, offsets, lens, pl):
    """Utterances 0 (33 frames), 1 (16) and 4 (20) start in slots 0..2 with reset flags; chunk 1 is 16
    frames of each; in chunk 2 slot 1 is refilled with utterance 2 (17 frames, reset) while slots 0 and 2
    carry on (17 and 4 frames).  -> {utterance: tokens}."""
    S = NP
    enc, dec = (eng.encode_stream_pl, eng.decode_stream_pl) if pl else (eng.encode_stream, eng.decode_stream)
    res = torch.empty((S, eng.max_res), dtype=torch.int32, device="cuda")
    rl = torch.zeros(S, dtype=torch.int32, device="cuda")
    got = {}
    rounds = [  # (slot, utterance, first frame, frames, reset)
        [(0, 0, 0, 16, 1), (1, 1, 0, 16, 1), (2, 4, 0, 16, 1)],
        [(0, 0, 16, 17, 0), (1, 2, 0, 17, 1), (2, 4, 16, 4, 0)],
    ]
    for rnd in rounds:
        off, cl, rs = np.zeros(S, np.int64), np.zeros(S, np.int32), np.zeros(S, np.int32)
        for slot, u, t0, k, r in rnd:
            off[slot], cl[slot], rs[slot] = offsets[u] + t0, k, r
        rd = torch.from_numpy(rs).cuda()
        enc(store, torch.from_numpy(off).cuda(), torch.from_numpy(cl).cuda(), cl, rd, int(cl.max()), S, S)
        dec(res, rl, rd)
        torch.cuda.synchronize()
        rlh = rl.cpu().numpy()
        for slot, u, t0, k, _ in rnd:
            if t0 + k == lens[u]:
                got[u] = res[slot, : rlh[slot]].cpu().numpy()
    return got


@pytest.mark.parametrize("pl", [False, True], ids=["rounds", "pipelined_calls"])
def test_stream_chunks_from_int8_store(pm, data, pl):
    e = Engine(pm, device=0, max_batch=NP, max_frames=64)  # its own: pipelined mode is for good
    try:
        sq = e.quantize(data["store"])
        f32 = _stream_tokens(e, data["store"], data["offsets"], data["lens"], pl)
        q8 = _stream_tokens(e, sq, data["offsets"], data["lens"], pl)
    finally:
        e.close()
    assert sorted(q8) == [0, 1, 2, 4]
    for u in q8:
        np.testing.assert_array_equal(q8[u], f32[u], err_msg=f"utterance {u} vs the fp32 stream")
        np.testing.assert_array_equal(q8[u], data["want"][u], err_msg=f"utterance {u} vs the restatement")


def test_misaligned_store_is_refused_before_any_launch(eng, data):
    lens_d, off_d = _batch(data)
    sq = eng.quantize(data["store"])
    rows = sq.shape[0] - 1
    shifted = sq.view(-1)[8: 8 + rows * 240].view(rows, 240)  # 8 bytes into the allocation
    assert shifted.is_contiguous() and shifted.data_ptr() % 16 == 8
    torch.cuda.synchronize()
    before = eng.stats(reset=False)
    reset = torch.zeros(NP, dtype=torch.int32, device="cuda")
    for call in (lambda: eng.encode_gather(shifted, off_d, lens_d, data["lens"], T, N, NP),
                 lambda: eng.encode_stream(shifted, off_d, lens_d, data["lens"], reset, T, N, NP),
                 lambda: eng.encode_stream_pl(shifted, off_d, lens_d, data["lens"], reset, T, N, NP),
                 lambda: eng.encode(shifted.view(-1)[: 256 * 256].view(1, 256, 256), lens_d, None, n=N)):
        with pytest.raises(EngineError, match=r"\(-22\).*16-byte aligned"):
            call()
    after = eng.stats(reset=False)
    assert after["encode_calls"] == before["encode_calls"] and after["step_launches"] == before["step_launches"]
    # and the engine still serves the round-form calls (the refused pipelined call left its mode alone)
    eng.encode_gather(sq, off_d, lens_d, data["lens"], T, N, NP)
    torch.cuda.synchronize()


def _offline_responses(pm, qsl, count):
    engines = [Engine(pm, device=0, max_batch=NP, max_frames=64)]
    try:
        sut = OfflineSUT(engines, qsl, batch_size=24)
        ids, idx = dist.query_arrays(count, count)
        sut.issue_batches(make_batches(qsl, ids, idx, 24))
        torch.cuda.synchronize()
        got_ids, lens, toks = sut.take_completed()
    finally:
        for e in engines:
            e.close()
    resp, off = {}, 0
    for sid, L in zip(got_ids, lens):
        resp[int(sid)] = toks[off: off + int(L)]
        off += int(L)
    return resp


def test_quantized_qsl_through_offline_sut(pm, eng):
    count = 60
    lengths = np.random.default_rng(8).integers(1, 41, count).astype(np.int32)
    qsl = GpuQSL(lengths, seed=8, device="cuda")
    q8 = qsl.quantized(eng)
    assert q8.feats.dtype == torch.int8 and q8.feats.shape == qsl.feats.shape
    assert q8.feats.numel() * q8.feats.element_size() * 4 == qsl.feats.numel() * qsl.feats.element_size()
    assert np.array_equal(q8.lengths, qsl.lengths) and np.array_equal(q8.offsets, qsl.offsets)
    want = _offline_responses(pm, qsl, count)
    got = _offline_responses(pm, q8, count)
    assert sorted(got) == list(range(count)) and sum(len(v) for v in want.values()) > 0
    for i in range(count):
        np.testing.assert_array_equal(got[i], want[i], err_msg=f"sample {i}")


def test_quantized_feature_store(eng):
    fs = FeatureStore(4, 8, device="cuda")
    fs.feats.copy_(torch.randn(fs.feats.shape, device="cuda") * 3)
    held = fs.alloc(2)
    q = fs.quantized(eng)
    assert q.feats.dtype == torch.int8 and q.feats.shape == fs.feats.shape and q.free == fs.free == 2
    assert (q.slots, q.max_frames, q.row(3)) == (fs.slots, fs.max_frames, fs.row(3))
    np.testing.assert_array_equal(q.feats.cpu().numpy(), eng.quantize_host(fs.feats.cpu().numpy()))
    q.release(held)  # its own bookkeeping
    assert q.free == 4 and fs.free == 2


# ---- the C++ drop-in with RNNT_HOST_Q8=1 (fixture recipe of tests/test_sut_harness_gpu.py)
def _responses(path):
    b = open(path, "rb").read()
    out, off = {}, 0
    while off < len(b):
        sid, size = np.frombuffer(b, np.int32, 2, off)
        off += 8
        assert int(sid) not in out, f"sample {sid} answered twice"
        out[int(sid)] = np.frombuffer(b, np.int32, int(size) // 4, off).copy()
        off += int(size)
    return out


@pytest.fixture(scope="module")
def harness_setup(tmp_path_factory, oracle):
    tmp = tmp_path_factory.mktemp("harness_q8")
    pm, _ = weights.build_model()
    eng_file = weights.save_engine_file(pm, str(tmp / "rnnt.engine"))
    rng = np.random.default_rng(61)
    lens = rng.integers(1, 62, 40).astype(np.int32)
    lens[[3, 17]] = [0, 61]
    lens[[5, 9, 22]] = [1, 2, 33]
    n, t = len(lens), int(lens.max())
    x = synthetic.make_features(t, n, seed=24, lens=lens)[:, :, :240]  # [T][N][240]
    ragged = np.concatenate([x[: lens[i], i] for i in range(n)])  # the QSL's frames back to back
    ragged.astype(np.float32).tofile(tmp / "feats.bin")
    lens.tofile(tmp / "lens.bin")
    fo = oracle.encoder_i8(pm, np.pad(x, ((0, 0), (0, 0), (0, 16))), lens)
    ro, rlo, _ = oracle.greedy_decode(pm, fo, (lens + 1) // 2, max_res=(500 // 2) * 30)
    assert rlo.max() > 3 and rlo[3] == 0
    query = np.array([i for i in range(n) if lens[i] > 0], np.int32)  # the Server answers no empty sample
    query.tofile(tmp / "query_server.bin")
    return dict(tmp=tmp, eng=eng_file, lens=lens, query=query, want=[ro[i, : rlo[i]] for i in range(n)])


def _run_harness(setup, name, host_q8, **kw):
    tmp = setup["tmp"]
    out = tmp / f"{name}.bin"
    cmd = [HARNESS, "--engine", setup["eng"], "--feats", str(tmp / "feats.bin"), "--lens", str(tmp / "lens.bin"),
           "--out", str(out)]
    for k, v in kw.items():
        cmd += ["--" + k.replace("_", "-"), str(v)]
    env = {k: v for k, v in os.environ.items() if k != "RNNT_HOST_Q8"}
    if host_q8:
        env["RNNT_HOST_Q8"] = "1"
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    summary = json.loads(r.stdout.strip().splitlines()[-1])
    assert summary["bad_sos_fill_rows"] == 0 and summary["bad_res_idx_rows"] == 0, summary
    return summary, _responses(out)


@pytest.mark.parametrize("host_q8,threads,split_len", [(1, 1, -1), (1, 8, 2), (0, 1, -1)],
                         ids=["q8_whole", "q8_split2", "env_unset"])
def test_harness_offline_host_q8(harness_setup, host_q8, threads, split_len):
    assert os.path.exists(HARNESS), "harness not built (make -C rnnt-inference_amd/csrc)"
    s = harness_setup
    n = len(s["lens"])
    summary, got = _run_harness(s, f"off_{host_q8}_{threads}_{split_len}", host_q8, scenario="offline",
                                threads=threads, batch=6, split_len=split_len, warmup=1 if threads == 8 else 0, intra=2)
    mh = summary["model_host_seconds"]
    assert mh["encode_calls"] == summary["batches"] == -(-n // 6), summary
    assert mh["q8_calls"] == (mh["encode_calls"] if host_q8 else 0), summary
    assert sorted(got) == list(range(n))
    for i in range(n):
        np.testing.assert_array_equal(got[i], s["want"][i], err_msg=f"sample {i}")


def test_harness_server_host_q8(harness_setup):
    s = harness_setup
    summary, got = _run_harness(s, "srv_q8", 1, scenario="server", threads=2, batch=16, split_len=2, response=16,
                                pro_batch=4, query=s["tmp"] / "query_server.bin", intra=2)
    mh = summary["model_host_seconds"]
    assert mh["encode_calls"] > 0 and mh["q8_calls"] == mh["encode_calls"], summary
    assert summary["responses"] == len(s["query"]) and sorted(got) == list(range(len(s["query"])))
    for pos, i in enumerate(s["query"]):
        np.testing.assert_array_equal(got[pos], s["want"][i], err_msg=f"query position {pos} (sample {i})")
