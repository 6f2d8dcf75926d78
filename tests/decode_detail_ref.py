"""Reference for the detail decode (Engine.decode(..., frames=, conf=)): the greedy loop of the
reference's decoder.py:125-167 walked in numpy over the CPU restatement's prediction and joint
(oracle.prediction / oracle.joint), recording for every emitted token the encoder frame the row
stood on and the confidence DESIGN.md section 2 defines:

    conf = 1 / S,  S = sum over the 29 labels of oracle_exp(v_j - v_best)   (float32 throughout)

summed as a fixed balanced tree -- "lane" l of 16 adds labels 2l and 2l+1 (slots 29..31 are exactly
0), then an xor butterfly over offsets 1, 2, 4, 8.  A plain module (not a conftest): the GPU tests
and the seed choice share it.  Its tokens must equal oracle.greedy_decode's, which ties it to the
committed oracle.  replay_steps / replay_decode also return every step's 29 logits (the edge-model
tests read them)."""
import ctypes as C

import numpy as np

NLAB, BLANK, SOS, MAXSYM = 29, 28, -1, 30


def confidence(oracle, v, best):
    """v: float32 [29] logits -> float32 confidence of label `best`."""
    exp = oracle.lib().oracle_exp
    v = np.asarray(v, np.float32)
    e = np.zeros(32, np.float32)
    for j in range(NLAB):
        e[j] = np.float32(exp(C.c_float(v[j] - v[best])))
    s = e[0::2] + e[1::2]  # float32 [16]
    lanes = np.arange(16)
    for off in (1, 2, 4, 8):
        s = s + s[lanes ^ off]
    assert s.dtype == np.float32
    return np.float32(1.0) / s[0]


def replay(oracle, pm, f, f_lens, max_res):
    """f [Tp, N, 1024] float32 (the restatement's encoder output), f_lens [N] ->
    (tokens, frames, conf): per row, int32 / int32 / float32 arrays of the row's res_len entries.
    Rows advance in lock step, so each step is one batched prediction and one batched joint."""
    return _walk(oracle, pm, f, f_lens, max_res)[:3]


def replay_steps(oracle, pm, f, f_lens, max_res):
    """replay's (tokens, frames, conf) + (logits, emitted): per row, every joint evaluation of the
    row in order -- logits float32 [steps, 29] and emitted int32 [steps], the label the step emitted
    (also when the token fell past max_res) or -1 where the row advanced (a blank, or the advance
    forced after MAXSYM symbols).  What the edge-model tests (joint_edge_models.py) read to show
    that a decode reached its edge."""
    return _walk(oracle, pm, f, f_lens, max_res)[:5]


def replay_decode(oracle, pm, f, f_lens, max_res):
    """replay_steps' five + (res, res_len) of the oracle.greedy_decode call the replay checks its tokens
    against (res [N, max_res] with the -1 fill; res_len = res_idx + 1, which counts tokens past max_res)."""
    return _walk(oracle, pm, f, f_lens, max_res)


def _walk(oracle, pm, f, f_lens, max_res):
    f = np.ascontiguousarray(f, np.float32)
    f_lens = np.asarray(f_lens, np.int32)
    N = f.shape[1]
    h = np.zeros((2, N, 320), np.float32)
    c = np.zeros((2, N, 320), np.float32)
    hn, cn = h.copy(), c.copy()
    g = np.zeros((N, 320), np.float32)
    pre_g = np.full(N, SOS, np.int32)
    time = np.zeros(N, np.int64)
    added = np.zeros(N, np.int64)
    cand = np.zeros(N, bool)
    live = f_lens > 0
    toks, frs, cfs = [[] for _ in range(N)], [[] for _ in range(N)], [[] for _ in range(N)]
    lgs, ems = [[] for _ in range(N)], [[] for _ in range(N)]
    while live.any():
        need = np.flatnonzero(live & ~cand)
        if len(need):
            gg, hh, cc = oracle.prediction(pm, pre_g[need], h[:, need], c[:, need])
            g[need], hn[:, need], cn[:, need] = gg, hh, cc
            cand[need] = True
        rows = np.flatnonzero(live)
        logits = oracle.joint(pm, f[time[rows], rows], g[rows])
        for k, n in enumerate(rows):
            v = logits[k]
            best = int(np.argmax(v))  # the first maximum, as torch.argmax
            lgs[n].append(v.copy())
            ems[n].append(best if best != BLANK and added[n] != MAXSYM else -1)
            if best != BLANK and added[n] != MAXSYM:
                if len(toks[n]) < max_res:
                    toks[n].append(best)
                    frs[n].append(int(time[n]))
                    cfs[n].append(confidence(oracle, v, best))
                added[n] += 1
                pre_g[n] = best
                h[:, n], c[:, n] = hn[:, n], cn[:, n]  # the candidate state is committed
                cand[n] = False
            else:  # blank, or the advance forced after MAXSYM symbols: next frame, same prediction
                time[n] += 1
                added[n] = 0
                if time[n] >= f_lens[n]:
                    live[n] = False
    ro, rlo, _ = oracle.greedy_decode(pm, f, f_lens, max_res=max_res)
    for n in range(N):
        k = min(int(rlo[n]), max_res)  # res_len = res_idx + 1 counts the tokens that fell past max_res too
        assert len(toks[n]) == k and np.array_equal(toks[n], ro[n, :k]), f"replay tokens differ, row {n}"
    return ([np.asarray(t, np.int32) for t in toks], [np.asarray(t, np.int32) for t in frs],
            [np.asarray(t, np.float32) for t in cfs],
            [np.asarray(t, np.float32).reshape(-1, NLAB) for t in lgs], [np.asarray(t, np.int32) for t in ems], ro, rlo)
