"""Joints that put the greedy decode on its decision edges: exact
ties between labels, between a label and blank, an all-negative maximum, a 29-way tie with an all-zero
joint hidden, and exp terms below det_exp's lower clamp.  The synthetic recipes never get there (their
blank bias is +7 .. +13 and their W2 rows are random), so the argmax's tie rule, its masking of the pad
slots 29..31 and the ends of the confidence tree would otherwise go unchecked.

Every model is `weights.build_model()`'s joint with a few arrays edited; the encoder and the prediction
network are untouched.  An edit is written once, on a view of the six joint arrays, and applied either
to a PreparedModel (`edge_model`) or to the checkpoint dict it was built from (`edge_checkpoint`, for
the fp32 decoder's `RNNT(ckpt, "f32")`).  The edits copy rows, add to fp32 biases or store small
constants, so bf16-held arrays stay bf16-representable and both forms describe the same joint
(`check_forms_agree`).  A plain module (not a conftest), like decode_detail_ref.py."""
import copy

import numpy as np

NLAB, BLANK = 29, 28
JOINT = ("w1t", "w1p", "bt", "bp", "w2", "b2")

# Labels made bit-identical (the W2 row and b2 of the first, a label the default decode emits often).
# The argmax gives lane l of 16 the labels 2l and 2l+1 and merges lanes by an xor butterfly over offsets
# 1, 2, 4, 8.  TIE_GROUP sits in lanes 0, 1, 2, 4, 8: with all five tied at the maximum, lane 0 meets an
# equal value from a larger label at every butterfly step.  TIE_PAIR shares lane 5 (the in-lane compare).
TIE_GROUP = (2, 0, 4, 8, 16)
TIE_PAIR = (10, 11)
# tie class -> (label that must win, the larger label it ties with)
TIE_CLASSES = {"lane": (10, 11), "xor1": (0, 2), "xor2": (0, 4), "xor4": (0, 8), "xor8": (0, 16)}
TIE_BLANK_DROP = 11.0  # blank bias 13 -> 2: the labels decide steps in all three joint tiles of the batch
BLANK_TIE_LABEL = 21  # the label the default joint ranks first among the non-blanks most often
NEGATIVE_SHIFT = -64.0
FLAT_B2 = -3.25
SPREAD_LABELS = (3, 12, 20)
SPREAD_SHIFT = -200.0


def _ties(j):
    for grp in (TIE_GROUP, TIE_PAIR):
        for lab in grp[1:]:
            j["w2"][lab] = j["w2"][grp[0]]
            j["b2"][lab] = j["b2"][grp[0]]
    j["b2"][BLANK] -= np.float32(TIE_BLANK_DROP)


def _blank_tie(j):
    j["w2"][BLANK] = j["w2"][BLANK_TIE_LABEL]
    j["b2"][BLANK] = j["b2"][BLANK_TIE_LABEL]


def _negative(j):
    _ties(j)
    j["b2"] += np.float32(NEGATIVE_SHIFT)


def _flat(j):
    j["w1t"][:] = 0
    j["w1p"][:] = 0
    j["bt"][:] = -1
    j["bp"][:] = 0
    j["b2"][:] = np.float32(FLAT_B2)


def _spread(j):
    j["b2"][BLANK] -= np.float32(TIE_BLANK_DROP)  # the short rows of the batch emit too
    j["b2"][list(SPREAD_LABELS)] += np.float32(SPREAD_SHIFT)


EDITS = {"TIES": _ties, "BLANK_TIE": _blank_tie, "NEGATIVE": _negative, "FLAT": _flat, "SPREAD": _spread}
NAMES = tuple(EDITS)


def edge_model(pm, name):
    """Deep copy of the PreparedModel `pm` with only the joint arrays edited."""
    out = copy.deepcopy(pm)
    j = {k: np.array(getattr(out, k), np.float32) for k in JOINT}
    EDITS[name](j)
    for k in JOINT:
        setattr(out, k, j[k])
    return out


def edge_checkpoint(ckpt, name):
    """The same edit on a checkpoint dict (original keys): joint_net.0 holds [W1t | W1p] and one
    bias (the migration gives it to the prediction half, the transcription half's is zero), joint_net.3
    W2 and b2."""
    out = {k: np.array(v, np.float32) for k, v in ckpt.items()}
    w1 = out["joint_net.0.weight"]
    H = w1.shape[1] - 320
    j = dict(w1t=w1[:, :H], w1p=w1[:, H:], bt=np.zeros(w1.shape[0], np.float32), bp=out["joint_net.0.bias"],
             w2=out["joint_net.3.weight"], b2=out["joint_net.3.bias"])
    EDITS[name](j)  # in place, through the views
    out["joint_net.0.bias"] = (j["bt"] + j["bp"]).astype(np.float32)
    return out


def check_forms_agree(pm, ckpt, name):
    """The edited checkpoint, rounded as prepare_model rounds it, is the edited PreparedModel's joint
    (the linear1 biases as their sum: the checkpoint holds one)."""
    from rnnt_amd import weights
    a, sd = edge_model(pm, name), weights.migrate_state_dict(edge_checkpoint(ckpt, name))
    cvt = weights.bf16_round if pm.bf16 else (lambda v: np.asarray(v, np.float32))
    for k, key in (("w1t", "joint.linear1_trans.weight"), ("w1p", "joint.linear1_pred.weight"), ("w2", "joint.linear2.weight")):
        np.testing.assert_array_equal(getattr(a, k).view(np.uint32), cvt(sd[key]).view(np.uint32), err_msg=f"{name} {k}")
    np.testing.assert_array_equal(a.b2, sd["joint.linear2.bias"], err_msg=f"{name} b2")
    np.testing.assert_array_equal(a.bt + a.bp, sd["joint.linear1_trans.bias"] + sd["joint.linear1_pred.bias"],
                                  err_msg=f"{name} linear1 bias")
    for k in ("embed", "amax", "enc_rb"):
        np.testing.assert_array_equal(getattr(a, k), getattr(pm, k))


# ---- what a decode of an edge model must contain (conditions on replay_steps' logits / emitted)
def max_ties(v):
    """Labels bit-equal to the row maximum of logits v [steps, 29] -> bool [steps, 29]."""
    v = np.asarray(v, np.float32)
    return v == v.max(1, keepdims=True)


def tie_counts(logits, emitted):
    """Per tie class: emitting steps whose winner and its larger twin are both at the maximum."""
    v = np.concatenate(logits)
    e = np.concatenate(emitted)
    top = max_ties(v)
    return {c: int((top[:, lo] & top[:, hi] & (e == lo)).sum()) for c, (lo, hi) in TIE_CLASSES.items()}


# ---- the batch every edge test decodes: the shape of test_decode_detail_gpu.py (40 rows in n_pad 256:
# two full 16-row joint tiles and a partial one; 24 feature frames = 12 encoder frames), lengths with 0,
# 1, odd ones, a full-length row, and the <= 8 / 9 / >= 17 frame utterances the stream case feeds in
# chunks of 8.  The other rows have 1 .. 4 frames: on BLANK_TIE and FLAT every encoder frame emits 30
# tokens, and the CPU restatement's bf16 prediction takes milliseconds per token.
N, NP, T = 40, 256, 24
SEED = 207


def edge_batch():
    """-> (lens int32 [N], x float32 [T, N, 256])."""
    from rnnt_amd import synthetic
    rng = np.random.default_rng(SEED)
    lens = rng.integers(1, 5, N).astype(np.int32)
    lens[[0, 1, 3, 5, 17]] = [24, 1, 9, 0, 17]
    return lens, synthetic.make_features(T, N, seed=SEED, lens=lens)
