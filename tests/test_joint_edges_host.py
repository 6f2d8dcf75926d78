"""The edge joints of tests/joint_edge_models.py on the CPU restatement alone (no GPU): each model's
decode of the shared batch reaches the edge it is built for, so the GPU comparisons of
test_joint_edges_gpu.py are not vacuous -- exact ties decided in the lane and at each of the four
butterfly steps, blank tied with the winning label, an all-negative maximum, the 29-way tie with its
confidence of exactly the tree's 1/29, exp terms below det_exp's clamp, the 30-symbol cap and tokens
past max_res.  The replay (decode_detail_ref.replay_steps) supplies the per-step logits and checks its
own tokens against oracle.greedy_decode for every model.

Counts observed when this file was written (batch of joint_edge_models.edge_batch, bf16 joint); the
assertions below only ask for "some", so a change of the synthetic recipe that empties a case fails here:
  TIES / NEGATIVE  739 tokens; decided ties: lane 40, xor1 131, xor2 131, xor4 131, xor8 131; 23 capped frames
  BLANK_TIE        2430 tokens on 2511 steps; blank at the maximum on 174 steps, never chosen; all 39
                   non-empty rows and all 81 frames capped
  FLAT             2430 tokens, all label 0, 2511 29-way ties, conf bits 0x3d0d3dcb (0.03448276)
  SPREAD           745 tokens, each with three terms below the clamp (v_j - v_best down to -227.7)
"""
import ctypes as C

import numpy as np
import pytest

import decode_detail_ref as ref
import joint_edge_models as jem
from rnnt_amd import weights

MAX_RES = 12 * 30
OVERFLOW_RES = 100
EXP_CLAMP = -87.0  # det_exp / oracle_exp clamp their argument below at -87


@pytest.fixture(scope="module")
def base(oracle):
    pm, ckpt = weights.build_model()
    lens, x = jem.edge_batch()
    return dict(pm=pm, ckpt=ckpt, lens=lens, fl=(lens + 1) // 2, fo=oracle.encoder_i8(pm, x, lens))


@pytest.fixture(scope="module")
def runs(base, oracle):
    cache = {}

    def run(name):
        if name not in cache:
            pm = jem.edge_model(base["pm"], name)
            toks, frs, cfs, lgs, ems = ref.replay_steps(oracle, pm, base["fo"], base["fl"], MAX_RES)  # == greedy_decode
            # advances forced by the cap: a non-blank argmax on a frame that already holds 30 symbols
            caps = np.array([int(((v[:, :28].max(1) >= v[:, 28]) & (_added_before(e) == ref.MAXSYM)).sum()) if len(e)
                             else 0 for v, e in zip(lgs, ems)])
            cache[name] = dict(pm=pm, toks=toks, frs=frs, cfs=cfs, lgs=lgs, ems=ems, caps=caps,
                               v=np.concatenate(lgs), e=np.concatenate(ems))
        return cache[name]
    return run


def test_batch_shape(base):
    lens = base["lens"]
    assert {0, 1, 9, 17, 24} <= set(lens.tolist()) and len(lens) == jem.N and lens.max() == jem.T


@pytest.mark.parametrize("name", jem.NAMES)
def test_only_the_joint_is_edited_and_both_forms_agree(base, name):
    pm, m = base["pm"], jem.edge_model(base["pm"], name)
    for k in weights._LISTS:
        for a, b in zip(getattr(pm, k), getattr(m, k)):
            np.testing.assert_array_equal(a, b)
    for k in weights._ARRAYS:
        if k not in jem.JOINT:
            np.testing.assert_array_equal(getattr(pm, k), getattr(m, k))
    for k in ("w1t", "w1p", "w2"):  # bf16-held arrays stay bf16-representable
        np.testing.assert_array_equal(getattr(m, k).view(np.uint32), weights.bf16_round(getattr(m, k)).view(np.uint32))
    assert any(not np.array_equal(getattr(pm, k), getattr(m, k)) for k in jem.JOINT)
    jem.check_forms_agree(pm, base["ckpt"], name)
    jem.check_forms_agree(weights.prepare_model(base["ckpt"], pm.amax, bf16=False), base["ckpt"], name)


@pytest.mark.parametrize("name", ["TIES", "NEGATIVE"])
def test_every_tie_class_decides_tokens(runs, name):
    r = runs(name)
    counts = jem.tie_counts(r["lgs"], r["ems"])
    print(name, "decided ties", counts, "tokens", int((r["e"] >= 0).sum()), "capped frames", int(r["caps"].sum()))
    for c, k in counts.items():
        assert k >= 1, f"{name}: no emitted token decided by a {c} tie ({counts})"
    losers = sorted(hi for _, hi in jem.TIE_CLASSES.values())  # 2, 4, 8, 11, 16
    assert not np.isin(r["e"], losers).any(), "a larger label of a tied group was emitted"
    # the twins are bit-equal on every step, whoever wins
    for grp in (sorted(jem.TIE_GROUP), list(jem.TIE_PAIR)):
        assert (r["v"][:, grp].view(np.uint32) == r["v"][:, grp[:1]].view(np.uint32)).all()


def test_negative_maximum_still_emits(runs):
    r = runs("NEGATIVE")
    assert (r["v"].max(1) < 0).all(), "a step has a non-negative logit"
    assert (r["e"] >= 0).sum() > 0
    # the shift leaves the decisions of TIES as they were: the same decode below zero
    t = runs("TIES")
    for a, b in zip(r["toks"], t["toks"]):
        np.testing.assert_array_equal(a, b)


def test_blank_tied_with_a_label_emits_the_label(runs):
    r = runs("BLANK_TIE")
    top = jem.max_ties(r["v"])
    tied = top[:, jem.BLANK]
    print("BLANK_TIE steps", len(tied), "blank at the maximum", int(tied.sum()), "tokens", int((r["e"] >= 0).sum()),
          "rows capped", int((r["caps"] > 0).sum()), "capped frames", int(r["caps"].sum()))
    assert tied.sum() >= 1, "blank never equals the maximum"
    assert (r["v"][:, jem.BLANK].view(np.uint32) == r["v"][:, jem.BLANK_TIE_LABEL].view(np.uint32)).all()
    assert (top[tied][:, jem.BLANK_TIE_LABEL]).all()
    # on such a step the row emits the label, or (30 symbols on the frame already) takes the forced advance
    added = np.concatenate([_added_before(e) for e in r["ems"]])
    assert ((r["e"][tied] == jem.BLANK_TIE_LABEL) | (added[tied] == ref.MAXSYM)).all(), "blank chosen on a tie"
    assert (r["e"][tied] == jem.BLANK_TIE_LABEL).sum() >= 1
    assert (r["e"][added < ref.MAXSYM] >= 0).all(), "blank won a step"
    assert (r["caps"] > 0).sum() >= 1, "no row hits the cap"


def _added_before(emitted):
    """symbols_added before each step of one row (emitted: replay_steps' per-row array)."""
    out, a = np.zeros(len(emitted), np.int64), 0
    for i, e in enumerate(emitted):
        out[i] = a
        a = a + 1 if e >= 0 else 0
    return out


def test_flat_joint_is_a_29_way_tie(runs, base, oracle):
    r = runs("FLAT")
    assert (r["v"].view(np.uint32) == np.float32(jem.FLAT_B2).view(np.uint32)).all(), "not every step is a 29-way tie"
    one29 = ref.confidence(oracle, np.full(29, jem.FLAT_B2, np.float32), 0)
    print("FLAT tokens", int((r["e"] >= 0).sum()), "conf", one29, hex(int(one29.view(np.uint32))))
    assert abs(float(one29) - 1.0 / 29.0) < 1e-8 and one29.view(np.uint32) == 0x3D0D3DCB
    for i, (t, f, c) in enumerate(zip(r["toks"], r["frs"], r["cfs"])):
        assert (t == 0).all()
        assert (c.view(np.uint32) == one29.view(np.uint32)).all()
        assert len(t) == ref.MAXSYM * base["fl"][i], f"row {i}: a frame does not end at the cap"
        if len(t):
            np.testing.assert_array_equal(np.bincount(f), np.full(base["fl"][i], ref.MAXSYM))
    np.testing.assert_array_equal(r["caps"], base["fl"])


def test_flat_overflow_reference_is_the_truncated_replay(runs, base, oracle):
    """With max_res below a row's token count the decode runs on and only the writes stop: the replay at
    max_res 100 (run here on rows 1 .. 4, one of them with 5 frames = 150 tokens) is the full replay cut at 100,
    which is what the GPU overflow test compares with; oracle.greedy_decode agrees."""
    r = runs("FLAT")
    rows = slice(1, 5)
    fo = np.ascontiguousarray(base["fo"][:, rows])
    toks, frs, cfs, _, ems = ref.replay_steps(oracle, r["pm"], fo, base["fl"][rows], OVERFLOW_RES)
    ro, rlo, _ = oracle.greedy_decode(r["pm"], fo, base["fl"][rows], max_res=OVERFLOW_RES)
    assert ro.shape[1] == OVERFLOW_RES
    assert sum(len(t) == OVERFLOW_RES for t in toks) >= 1 and min(len(t) for t in toks) == 30
    for i, row in enumerate(range(1, 5)):
        assert rlo[i] == len(r["toks"][row])  # res_len = res_idx + 1 counts what fell past max_res
        np.testing.assert_array_equal(toks[i], r["toks"][row][:OVERFLOW_RES])
        np.testing.assert_array_equal(frs[i], r["frs"][row][:OVERFLOW_RES])
        np.testing.assert_array_equal(cfs[i].view(np.uint32), r["cfs"][row][:OVERFLOW_RES].view(np.uint32))
        np.testing.assert_array_equal(ems[i], r["ems"][row])  # the steps go on past max_res


def test_spread_reaches_the_exp_clamp(runs, oracle):
    r = runs("SPREAD")
    d = r["v"] - r["v"].max(1, keepdims=True)
    hit = (d < np.float32(EXP_CLAMP)).any(1) & (r["e"] >= 0)
    print("SPREAD emitting steps with a clamped term", int(hit.sum()), "of", int((r["e"] >= 0).sum()), "min", float(d.min()))
    assert hit.sum() >= 1, "no emitting step has a term below the clamp"
    # the clamp: such a term is exp(-87), a normal float, not 0 and not a denormal
    exp = oracle.lib().oracle_exp
    lo = np.float32(exp(C.c_float(EXP_CLAMP)))
    assert np.float32(exp(C.c_float(float(d.min())))) == lo and lo >= np.finfo(np.float32).tiny
    assert all((c > 0).all() and (c <= 1).all() for c in r["cfs"])
