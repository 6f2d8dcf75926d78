"""The decode kernels on the edge joints of tests/joint_edge_models.py (exact ties in the lane and at each
butterfly step, blank tied with a label, an all-negative maximum, the 29-way tie at y1 = 0, exp terms
below the clamp, the cap on every frame, tokens past max_res), every comparison exact: the fused decode
and its detail joints against oracle.greedy_decode and the replay (decode_detail_ref), the persistent
tail, decode_stream, the op-by-op loop and the fp32 decoder.  tests/test_joint_edges_host.py shows on the
CPU that each model's decode of this batch reaches its edge.

One engine and one encode per model, module-scoped and made on first use; each is closed at the end."""
import numpy as np
import pytest
import torch

import decode_detail_ref as ref
import joint_edge_models as jem
from rnnt_amd import weights
from rnnt_amd.engine import Engine

pytestmark = pytest.mark.gpu

N, NP, T = jem.N, jem.NP, jem.T
FRAME_FILL, CONF_FILL = -77, -3.5  # sentinels: positions at or past res_len stay as they were
OVERFLOW_RES = 100
PERSIST_ROWS = 16  # the three long rows of the batch are what is left once the short ones have finished


@pytest.fixture(scope="module")
def base(oracle):
    pm, ckpt = weights.build_model()
    lens, x = jem.edge_batch()
    return dict(pm=pm, ckpt=ckpt, lens=lens, x=x, fl=(lens + 1) // 2, fo=oracle.encoder_i8(pm, x, lens))


def _bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _encode(eng, base):
    xp = np.zeros((T, NP, 256), np.float32)
    xp[:, :N] = base["x"]
    lp = np.zeros(NP, np.int32)
    lp[:N] = base["lens"]
    f = torch.zeros(((T + 1) // 2, NP, 1024), dtype=torch.float32, device="cuda")
    eng.encode(torch.from_numpy(xp).cuda(), torch.from_numpy(lp).cuda(), base["lens"], n=N, f_out=f)
    torch.cuda.synchronize()
    fg = f.cpu().numpy()
    for i in range(N):  # the decode comparisons rest on the encoder frames
        k = base["fl"][i]
        assert np.array_equal(fg[:k, i].view(np.uint32), base["fo"][:k, i].view(np.uint32)), f"encoder row {i}"


def _buffers(width, n=N, tail=0):
    """res, res_len, frames, conf of `width` columns; with `tail`, each detail array is a view of a
    longer sentinel-filled allocation whose last `tail` elements no row owns."""
    def mk(fill, dt):
        flat = torch.full((n * width + tail,), fill, dtype=dt, device="cuda")
        return flat, flat[: n * width].view(n, width)
    res = torch.empty((n, width), dtype=torch.int32, device="cuda")
    rl = torch.empty(n, dtype=torch.int32, device="cuda")
    (fr_all, fr), (cf_all, cf) = mk(FRAME_FILL, torch.int32), mk(CONF_FILL, torch.float32)
    return res, rl, fr, cf, fr_all, cf_all


def _plain(eng, width):
    res, rl = _buffers(width)[:2]
    eng.decode(res, rl)
    torch.cuda.synchronize()
    return res.cpu().numpy(), rl.cpu().numpy()


def _detail(eng, width, tail=0):
    res, rl, fr, cf, fr_all, cf_all = _buffers(width, tail=tail)
    eng.decode(res, rl, frames=fr, conf=cf)
    torch.cuda.synchronize()
    return (res.cpu().numpy(), rl.cpu().numpy(), fr.cpu().numpy(), cf.cpu().numpy(),
            fr_all.cpu().numpy()[N * width:], cf_all.cpu().numpy()[N * width:])


def _reference(oracle, pm, base, max_res):
    ro, rlo, _ = oracle.greedy_decode(pm, base["fo"], base["fl"], max_res=max_res)
    return ro, rlo


@pytest.fixture(scope="module")
def models(base, oracle):
    """name -> one edge model's engine with the batch encoded, the restatement's decode and the replay;
    made on first use, every engine closed when the module is done."""
    made = {}

    def get(name):
        if name not in made:
            pm = jem.edge_model(base["pm"], name)
            eng = Engine(pm, device=0, max_batch=NP, max_frames=32)
            made[name] = dict(name=name, pm=pm, eng=eng, memo={})
            _encode(eng, base)
            # ro, rlo: oracle.greedy_decode's res and res_len (the replay checks its tokens against them)
            toks, frs, cfs, lgs, ems, ro, rlo = ref.replay_decode(oracle, pm, base["fo"], base["fl"], eng.max_res)
            made[name].update(toks=toks, frs=frs, cfs=cfs, lgs=lgs, ems=ems, ro=ro, rlo=rlo)
        return made[name]
    yield get
    for m in made.values():
        m["eng"].close()


def _only(*names):
    return pytest.mark.parametrize("name", names)


def _offline(ctx):
    """The model's plain and detail decodes of the batch (run once)."""
    m = ctx["memo"]
    if "plain" not in m:
        m["plain"] = _plain(ctx["eng"], ctx["eng"].max_res)
        m["detail"] = _detail(ctx["eng"], ctx["eng"].max_res)
    return m["plain"], m["detail"]


def _check_detail(got, toks, frs, cfs, rlo, width):
    res, rl, fr, cf = got[:4]
    np.testing.assert_array_equal(rl, rlo)
    for i in range(N):
        k = min(int(rl[i]), width)
        assert k == len(toks[i])
        np.testing.assert_array_equal(res[i, :k], toks[i], err_msg=f"tokens, row {i}")
        assert (res[i, k:] == -1).all(), f"row {i}: res fill"
        np.testing.assert_array_equal(fr[i, :k], frs[i], err_msg=f"frames, row {i}")
        np.testing.assert_array_equal(cf[i, :k].view(np.uint32), cfs[i].view(np.uint32), err_msg=f"conf bits, row {i}")
        assert (fr[i, k:] == FRAME_FILL).all() and (cf[i, k:] == np.float32(CONF_FILL)).all(), f"row {i} written past res_len"


@_only(*jem.NAMES)
def test_plain_decode_equals_the_restatement(models, name):
    ctx = models(name)
    (res, rl), _ = _offline(ctx)
    assert ctx["rlo"].sum() > 0 and {0, 1, 9, 17, 24} <= set(jem.edge_batch()[0].tolist())
    np.testing.assert_array_equal(rl, ctx["rlo"])
    np.testing.assert_array_equal(res, ctx["ro"])  # the -1 fill included


@_only(*jem.NAMES)
def test_detail_decode_equals_the_replay(models, name):
    ctx = models(name)
    plain, det = _offline(ctx)
    np.testing.assert_array_equal(det[0], plain[0])
    np.testing.assert_array_equal(det[1], plain[1])
    _check_detail(det, ctx["toks"], ctx["frs"], ctx["cfs"], ctx["rlo"], ctx["eng"].max_res)
    if ctx["name"] == "FLAT":  # the 29-way tie: label 0 and the tree's 1/29 on every token
        k = int(det[1][0])
        assert k == 12 * 30 and (det[0][0, :k] == 0).all() and (det[3][0, :k].view(np.uint32) == 0x3D0D3DCB).all()


@_only(*jem.NAMES)
def test_persistent_tail_gives_the_same_tokens(models, name):
    """The persistent launch takes the run over once at most PERSIST_ROWS rows are live (it stops at
    the decode's last step, the four-launch loop at the end of a chunk); a detail decode ignores the
    setting and runs step launches to the end."""
    ctx = models(name)
    eng = ctx["eng"]
    plain, det = _offline(ctx)
    eng.stats(reset=True)
    _plain(eng, eng.max_res)
    loop_steps = eng.stats(reset=True)["decode_steps"]
    eng.set_decode_persist(PERSIST_ROWS)
    try:
        res, rl = _plain(eng, eng.max_res)
        tail_steps = eng.stats(reset=True)["decode_steps"]
        det2 = _detail(eng, eng.max_res)
    finally:
        eng.set_decode_persist(0)
    print(ctx["name"], "decode steps: loop", loop_steps, "with the persistent tail", tail_steps)
    np.testing.assert_array_equal(rl, plain[1])
    np.testing.assert_array_equal(res, plain[0])
    if ctx["name"] in ("BLANK_TIE", "FLAT"):  # 12 frames x 30 symbols: far past the two chunks before the first poll
        assert tail_steps < loop_steps, "the persistent launch did not take part"
    for a, b in zip(det2[:4], det[:4]):
        np.testing.assert_array_equal(_bits(a), _bits(b))


def _chunks(n):
    return [min(8, n), min(8, max(n - 8, 0)), max(n - 16, 0)]


@_only("TIES", "FLAT")
def test_stream_chunks_give_the_one_call_values(models, name, base):
    """Utterances fed as 8 + 8 + rest feature frames (test_decode_detail_gpu.py's chunking; slot 1 is
    reset with a new utterance at call 2): tokens, frames counted from the utterance's start, conf."""
    ctx = models(name)
    eng, lens = ctx["eng"], base["lens"]
    res0, rl0, fr0, cf0 = _offline(ctx)[1][:4]
    a = next(i for i in range(N) if lens[i] >= 17 and len(ctx["frs"][i]) and ctx["frs"][i].max() >= 8)
    d = next(i for i in range(N) if lens[i] >= 17 and i != a and rl0[i] > 0 and ctx["frs"][i].max() >= 4)
    b = next(i for i in range(N) if 0 < lens[i] <= 8)
    c = next(i for i in range(N) if 9 <= lens[i] <= 16 and rl0[i] > 0)
    assert ctx["frs"][a][-1] >= 8 and ctx["frs"][d][-1] >= 4, "no emission after a chunk boundary"
    order, offsets, rows, at = [a, b, c, d], {}, [], 0
    for u in order:
        offsets[u] = at
        rows.append(base["x"][: lens[u], u, :240])
        at += int(lens[u])
    store = torch.from_numpy(np.ascontiguousarray(np.concatenate(rows))).cuda()
    S = NP
    res, rl, fr, cf = _buffers(eng.max_res, S)[:4]
    calls = [[(0, a, 0, 1), (1, b, 0, 1), (2, d, 0, 1)],  # (slot, utterance, its chunk index, reset)
             [(0, a, 1, 0), (1, c, 0, 1), (2, d, 1, 0)],
             [(0, a, 2, 0), (1, c, 1, 0), (2, d, 2, 0)]]
    got = {}
    try:
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
    finally:
        _encode(eng, base)  # the engine's last encode is the batch again for the tests that follow
    assert sorted(got) == sorted(order)
    for u in order:
        n = int(rl0[u])
        np.testing.assert_array_equal(got[u][0], res0[u, :n], err_msg=f"tokens, utterance {u}")
        np.testing.assert_array_equal(got[u][1], fr0[u, :n], err_msg=f"frames, utterance {u}")
        np.testing.assert_array_equal(got[u][2].view(np.uint32), cf0[u, :n].view(np.uint32), err_msg=f"conf, utterance {u}")
        assert len(got[u][1]) == n and (np.diff(got[u][1]) >= 0).all()
    if ctx["name"] == "FLAT":  # every frame of the utterance, in order, across the chunk boundaries
        np.testing.assert_array_equal(got[a][1], np.repeat(np.arange((lens[a] + 1) // 2), 30))


@_only("TIES", "BLANK_TIE", "NEGATIVE")
def test_op_loop_equals_the_restatement(models, name, base, oracle):
    """TorchModel::decode's op loop on torch.ops.intel_mlperf (torch.argmax picks the symbol) with the
    edge model's reference-layout weights: res, res_idx + 1 and the -1 fill."""
    from rnnt_amd import ops
    from test_torch_ops_gpu import _decode, _eager_step, _encoder
    ctx = models(name)
    ops.load_library()
    W = ops.reference_weights(ctx["pm"], device="cpu")
    ld = torch.from_numpy(base["lens"]).cuda()
    f, _ = _encoder(W, torch.from_numpy(base["x"][:, :, :240].copy()).cuda(), ld)
    torch.cuda.synchronize()
    fg = f.cpu().numpy()
    for i in range(N):
        k = base["fl"][i]
        assert np.array_equal(fg[:k, i].view(np.uint32), base["fo"][:k, i].view(np.uint32)), f"encoder row {i}"
    st = _decode(W, f, ((ld + 1) // 2).to(torch.int32), _eager_step(W))
    ro, rlo, _ = oracle.greedy_decode(ops.op_model(ctx["pm"]), base["fo"], base["fl"], max_res=st["res"].shape[1])
    assert rlo.sum() > 0
    np.testing.assert_array_equal((st["res_idx"] + 1).cpu().numpy(), rlo)
    np.testing.assert_array_equal(st["res"].cpu().numpy(), ro)


@_only("TIES", "FLAT", "NEGATIVE")
def test_f32_decoder_equals_the_f32_restatement(name, base, oracle):
    """decoder_f32.hip (a serial first-maximum scan) on the same edit of the checkpoint: the tokens of
    the restatement's fp32 decode, whose logits tie as the bf16 ones do (bit-identical rows)."""
    from rnnt_amd.decoder import GreedyDecoder
    from rnnt_amd.model import RNNT
    m = RNNT(jem.edge_checkpoint(base["ckpt"], name), "f32", enable_bf16=False)
    x = base["x"][:, :, :240]
    fo = oracle.encoder_f32(m.f32_encoder_layers(), x, base["lens"])
    toks, _, _, lgs, ems = ref.replay_steps(oracle, m.pm32, fo, base["fl"], 30 * T)  # == greedy_decode(pm32)
    v, e = np.concatenate(lgs), np.concatenate(ems)
    if name == "FLAT":
        assert (v.view(np.uint32) == np.float32(jem.FLAT_B2).view(np.uint32)).all() and (e[e >= 0] == 0).all()
    else:
        counts = jem.tie_counts(lgs, ems)
        print(name, "fp32 decided ties", counts, "tokens", int((e >= 0).sum()))
        assert min(counts.values()) >= 1, counts
        assert not np.isin(e, [hi for _, hi in jem.TIE_CLASSES.values()]).any()
    if name == "NEGATIVE":
        assert (v.max(1) < 0).all() and (e >= 0).sum() > 0
    dec = GreedyDecoder(m, "f32", False, batch_size=N, max_frames=32)
    try:
        res, rl = dec(torch.from_numpy(np.ascontiguousarray(x)).cuda(), torch.from_numpy(base["lens"]))
        torch.cuda.synchronize()
        res, rl = res.cpu().numpy(), rl.cpu().numpy()
    finally:
        dec.close()
    np.testing.assert_array_equal(rl, [len(t) for t in toks])
    for i in range(N):
        np.testing.assert_array_equal(res[i, : rl[i]], toks[i], err_msg=f"row {i}")
        assert (res[i, rl[i]:] == -1).all()


@_only("FLAT")
def test_overflow_writes_nothing_at_or_past_max_res(models, name, base, oracle):
    """An engine with max_res 100 < 12 x 30: the decode runs on (res_len = res_idx + 1 counts every
    token), the writes stop at column 100.  The replay at max_res 100 is the full replay cut there
    (test_joint_edges_host.py).  frames / conf must have res's shape, so each is a view of a longer
    allocation: a write past a row's end lands in the next row's sentinels or values, one past the last
    row in the tail."""
    ctx = models(name)
    eng = Engine(ctx["pm"], device=0, max_batch=NP, max_frames=32, max_res=OVERFLOW_RES)
    try:
        assert eng.max_res == OVERFLOW_RES
        _encode(eng, base)
        res, rl = _plain(eng, OVERFLOW_RES)
        det = _detail(eng, OVERFLOW_RES, tail=4096)
    finally:
        eng.close()
    ro, rlo = _reference(oracle, ctx["pm"], base, OVERFLOW_RES)
    assert (rlo > OVERFLOW_RES).sum() >= 3 and (rlo == 30 * base["fl"]).all()
    np.testing.assert_array_equal(rl, rlo)
    np.testing.assert_array_equal(res, ro)
    np.testing.assert_array_equal(det[0], ro)
    cut = [[a[:OVERFLOW_RES] for a in ctx[k]] for k in ("toks", "frs", "cfs")]
    _check_detail(det, *cut, rlo, OVERFLOW_RES)
    assert (det[4] == FRAME_FILL).all() and (det[5] == np.float32(CONF_FILL)).all(), "written past the last row"
