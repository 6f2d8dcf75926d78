"""Detail decode on the GPU: Engine.decode / decode_stream with frames= and conf= against the numpy
replay of the greedy loop (tests/decode_detail_ref.py), bit for bit -- conf compared as uint32.

One engine and one 40-row batch (n_pad 256, 24 feature frames = 12 encoder frames) per module; the
seed was chosen on the CPU with the replay so that the batch has a frame carrying two or more tokens,
a blank advance between two emissions, tokens in all three 16-row joint tiles, and utterances the
stream case needs (asserted below, so the tests cannot pass vacuously).  The cap case runs on the cap
checkpoint of tests/test_cap_gpu.py (the golden model's prior never reaches the 30-symbol cap)."""
import ctypes as C

import numpy as np
import pytest
import torch

import decode_detail_ref as ref
from rnnt_amd import _lib, synthetic
from rnnt_amd.engine import Engine
from test_cap_gpu import _cap_input, cap_ckpt, cap_pm  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

N, NP, T = 40, 256, 24
SEED = 207  # chosen with the replay (module docstring): 97 tokens; rows 17 and 39 emit in their third chunk
FRAME_FILL, CONF_FILL = -77, -3.5  # sentinels: positions at or past res_len stay as they were


def _lens(seed):
    rng = np.random.default_rng(seed)
    lens = rng.integers(2, T + 1, N).astype(np.int32)
    lens[[0, 1, 2, 3, 17, 33, 39]] = [24, 1, 23, 16, 24, 8, 21]  # full, 1, odd, ...
    lens[5] = 0
    return lens


@pytest.fixture(scope="module")
def batch(pm_golden, oracle):
    lens = _lens(SEED)
    x = synthetic.make_features(T, N, seed=SEED, lens=lens)  # [T][N][256]
    fo = oracle.encoder_i8(pm_golden, x, lens)
    fl = (lens + 1) // 2
    toks, frs, cfs = ref.replay(oracle, pm_golden, fo, fl, max_res=16 * 30)
    return dict(lens=lens, x=x, fo=fo, fl=fl, toks=toks, frs=frs, cfs=cfs)


@pytest.fixture(scope="module")
def eng(pm_golden):
    e = Engine(pm_golden, device=0, max_batch=NP, max_frames=32)
    yield e
    e.close()


def _encode(eng, batch):
    xp = np.zeros((T, NP, 256), np.float32)
    xp[:, :N] = batch["x"]
    lp = np.zeros(NP, np.int32)
    lp[:N] = batch["lens"]
    eng.encode(torch.from_numpy(xp).cuda(), torch.from_numpy(lp).cuda(), batch["lens"], n=N)


def _buffers(eng, n=N):
    res = torch.empty((n, eng.max_res), dtype=torch.int32, device="cuda")
    rl = torch.empty(n, dtype=torch.int32, device="cuda")
    fr = torch.full((n, eng.max_res), FRAME_FILL, dtype=torch.int32, device="cuda")
    cf = torch.full((n, eng.max_res), CONF_FILL, dtype=torch.float32, device="cuda")
    return res, rl, fr, cf


def _detail(eng, frames=True, conf=True):
    """Detail decode of the engine's last encode -> host (res, res_len, frames, conf)."""
    res, rl, fr, cf = _buffers(eng)
    eng.decode(res, rl, frames=fr if frames else None, conf=cf if conf else None)
    torch.cuda.synchronize()
    return res.cpu().numpy(), rl.cpu().numpy(), fr.cpu().numpy(), cf.cpu().numpy()


@pytest.fixture(scope="module")
def offline(eng, batch):
    _encode(eng, batch)
    plain_res, plain_rl, _, _ = _buffers(eng)
    eng.decode(plain_res, plain_rl)
    torch.cuda.synchronize()
    return dict(plain=(plain_res.cpu().numpy(), plain_rl.cpu().numpy()), detail=_detail(eng))


def test_offline_frames_and_confidences_equal_the_replay(eng, batch, offline, pm_golden, oracle):
    toks, frs, cfs, fl = batch["toks"], batch["frs"], batch["cfs"], batch["fl"]
    # the batch exercises what it is meant to (module docstring)
    assert any(len(f) and np.bincount(f).max() >= 2 for f in frs), "no frame carries two tokens"
    assert any(len(f) > 1 and (np.diff(f) >= 2).any() for f in frs), "no blank advance between two emissions"
    assert all(sum(len(t) for t in toks[a:b]) > 0 for a, b in ((0, 16), (16, 32), (32, 40))), "a joint tile emits nothing"
    assert {1, 23, 24, 0} <= set(batch["lens"].tolist())
    res, rl, fr, cf = offline["detail"]
    np.testing.assert_array_equal(rl, [len(t) for t in toks])
    np.testing.assert_array_equal(rl, offline["plain"][1])
    np.testing.assert_array_equal(res, offline["plain"][0])
    ro, rlo, _ = oracle.greedy_decode(pm_golden, batch["fo"], fl, max_res=eng.max_res)
    np.testing.assert_array_equal(rl, rlo)
    np.testing.assert_array_equal(res, ro)
    for i in range(N):
        k = int(rl[i])
        np.testing.assert_array_equal(fr[i, :k], frs[i], err_msg=f"frames, row {i}")
        np.testing.assert_array_equal(cf[i, :k].view(np.uint32), cfs[i].view(np.uint32), err_msg=f"conf bits, row {i}")
        assert (fr[i, k:] == FRAME_FILL).all() and (cf[i, k:] == np.float32(CONF_FILL)).all(), f"row {i} written past res_len"
        if k:
            assert (np.diff(fr[i, :k]) >= 0).all() and 0 <= fr[i, 0] and fr[i, k - 1] < fl[i], f"row {i} frames"
            assert (cf[i, :k] > 0).all() and (cf[i, :k] <= 1).all(), f"row {i} conf range"


def test_null_combinations(eng, batch, offline):
    res, rl, fr, cf = offline["detail"]
    r1, l1, f1, c1 = _detail(eng, conf=False)  # frames only
    np.testing.assert_array_equal(r1, res)
    np.testing.assert_array_equal(l1, rl)
    np.testing.assert_array_equal(f1, fr)
    assert (c1 == np.float32(CONF_FILL)).all()
    r2, l2, f2, c2 = _detail(eng, frames=False)  # conf only
    np.testing.assert_array_equal(r2, res)
    np.testing.assert_array_equal(l2, rl)
    np.testing.assert_array_equal(c2.view(np.uint32), cf.view(np.uint32))
    assert (f2 == FRAME_FILL).all()
    # both null through the C entry: the plain decode
    r3, l3, _, _ = _buffers(eng)
    rc = eng._lib.rnnt_engine_decode_detail(eng._h, r3.data_ptr(), l3.data_ptr(), r3.shape[1], None, None,
                                            C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    np.testing.assert_array_equal(r3.cpu().numpy(), offline["plain"][0])
    np.testing.assert_array_equal(l3.cpu().numpy(), offline["plain"][1])


def test_persistent_tail_setting_is_ignored(eng, batch, offline):
    eng.set_decode_persist(64)
    try:
        got = _detail(eng)
    finally:
        eng.set_decode_persist(0)
    for a, b in zip(got, offline["detail"]):
        np.testing.assert_array_equal(a.view(np.uint32) if a.dtype == np.float32 else a,
                                      b.view(np.uint32) if b.dtype == np.float32 else b)


def _chunks(n):
    return [min(8, n), min(8, max(n - 8, 0)), max(n - 16, 0)]


def test_stream_chunks_carry_the_frame_base(eng, batch, offline):
    """Utterances fed as 8 + 8 + rest feature frames; slot 1's first utterance ends in call 1 and the slot
    is reset with a new one at call 2.  Per utterance: the one-call detail decode's values."""
    lens, frs = batch["lens"], batch["frs"]
    res0, rl0, fr0, cf0 = offline["detail"]
    long_rows = [i for i in range(N) if lens[i] >= 17 and len(frs[i]) and frs[i].max() >= 8]
    assert len(long_rows) >= 1, "no utterance emits in its third chunk"
    a = long_rows[0]
    d = next(i for i in range(N) if lens[i] >= 17 and i != a and rl0[i] > 0)
    b = next(i for i in range(N) if 0 < lens[i] <= 8)
    c = next(i for i in range(N) if 9 <= lens[i] <= 16 and rl0[i] > 0)  # emits: a stale frame base would show
    # ragged store of the four utterances' frames
    order, offsets, rows, at = [a, b, c, d], {}, [], 0
    for u in order:
        offsets[u] = at
        rows.append(batch["x"][: lens[u], u, :240])
        at += int(lens[u])
    store = torch.from_numpy(np.ascontiguousarray(np.concatenate(rows))).cuda()
    S = NP
    res, rl, fr, cf = _buffers(eng, S)
    # (slot, utterance, its chunk index, reset)
    calls = [[(0, a, 0, 1), (1, b, 0, 1), (2, d, 0, 1)],
             [(0, a, 1, 0), (1, c, 0, 1), (2, d, 1, 0)],
             [(0, a, 2, 0), (1, c, 1, 0), (2, d, 2, 0)]]
    got = {}
    for call in calls:
        off, cl, rs = np.zeros(S, np.int64), np.zeros(S, np.int32), np.zeros(S, np.int32)
        for slot, u, k, r in call:
            ch = _chunks(int(lens[u]))
            off[slot], cl[slot], rs[slot] = offsets[u] + sum(ch[:k]), ch[k], r
        rd = torch.from_numpy(rs).cuda()
        eng.encode_stream(store, torch.from_numpy(off).cuda(), torch.from_numpy(cl).cuda(), cl, rd, int(cl.max()), S, S)
        eng.decode_stream(res, rl, rd, frames=fr, conf=cf)
        torch.cuda.synchronize()
        rlh = rl.cpu().numpy()
        for slot, u, k, _ in call:
            if sum(_chunks(int(lens[u]))[: k + 1]) == lens[u] and u not in got:
                n = int(rlh[slot])
                got[u] = (res[slot, :n].cpu().numpy(), fr[slot, :n].cpu().numpy(), cf[slot, :n].cpu().numpy())
    assert sorted(got) == sorted(order)
    for u in order:
        n = int(rl0[u])
        np.testing.assert_array_equal(got[u][0], res0[u, :n], err_msg=f"tokens, utterance {u}")
        np.testing.assert_array_equal(got[u][1], fr0[u, :n], err_msg=f"frames, utterance {u}")
        np.testing.assert_array_equal(got[u][2].view(np.uint32), cf0[u, :n].view(np.uint32), err_msg=f"conf, utterance {u}")


def test_detail_call_before_any_encode_is_refused(pm_golden):
    e = Engine(pm_golden, device=0, max_batch=NP, max_frames=32)
    try:
        res, rl, fr, cf = _buffers(e)
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        rc = e._lib.rnnt_engine_decode_detail(e._h, res.data_ptr(), rl.data_ptr(), res.shape[1], fr.data_ptr(),
                                              cf.data_ptr(), st)
        assert rc == _lib.RNNT_EINVAL
        reset = torch.ones(NP, dtype=torch.int32, device="cuda")
        rc = e._lib.rnnt_engine_decode_stream_detail(e._h, res.data_ptr(), rl.data_ptr(), res.shape[1],
                                                     reset.data_ptr(), fr.data_ptr(), cf.data_ptr(), st)
        assert rc == _lib.RNNT_EINVAL
        with pytest.raises(_lib.EngineError, match=r"\(-22\)"):
            e.decode(res, rl, frames=fr, conf=cf)
    finally:
        e.close()


def test_capped_frame_shares_one_frame_value(cap_pm, golden, oracle):  # noqa: F811
    """On the cap checkpoint a frame emits max_symbols_per_step tokens and is then left by a forced
    advance: its 30 tokens carry one frame value and the next token a larger one."""
    x, lens = _cap_input(golden)
    n, Tc = len(lens), x.shape[0]
    xp = np.zeros((Tc, NP, 256), np.float32)
    xp[:, :n] = x
    lp = np.zeros(NP, np.int32)
    lp[:n] = lens
    e = Engine(cap_pm, device=0, max_batch=NP, max_frames=64)
    try:
        res, rl, fr, cf = _buffers(e, n)
        e.encode(torch.from_numpy(xp).cuda(), torch.from_numpy(lp).cuda(), lens, n=n)
        e.decode(res, rl, frames=fr, conf=cf)
        torch.cuda.synchronize()
        res, rl, fr, cf = res.cpu().numpy(), rl.cpu().numpy(), fr.cpu().numpy(), cf.cpu().numpy()
    finally:
        e.close()
    fo = oracle.encoder_i8(cap_pm, x, lens)
    ro, rlo, _, caps = oracle.greedy_decode_caps(cap_pm, fo, (lens + 1) // 2, max_res=res.shape[1])
    assert (caps > 0).sum() >= 3, f"the input does not reach the cap: {caps}"
    np.testing.assert_array_equal(rl, rlo)
    np.testing.assert_array_equal(res, ro)
    followed = 0
    for i in np.flatnonzero(caps > 0):
        k = int(rl[i])
        f = fr[i, :k]
        assert (np.diff(f) >= 0).all() and f[-1] < (lens[i] + 1) // 2
        assert (cf[i, :k] > 0).all() and (cf[i, :k] <= 1).all()
        counts = np.bincount(f)
        assert counts.max() == 30, f"row {i}: no frame carries exactly 30 tokens ({counts})"
        assert int((counts == 30).sum()) >= int(caps[i]), (i, counts, caps[i])
        for t in np.flatnonzero(counts == 30):
            last = int(np.flatnonzero(f == t)[-1])
            if last + 1 < k:
                assert f[last + 1] > t
                followed += 1
    assert followed > 0, "no capped frame is followed by a token"
