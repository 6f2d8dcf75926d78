"""Word timestamps and confidences from a detail decode (Engine.decode(..., frames=, conf=),
GreedyDecoder.forward(..., details=True)).

A token's frame is the encoder output frame the greedy loop stood on when it emitted the token;
one such frame covers ``config.FRAME_SECONDS`` of audio (10 ms hop x splicing 3 x stacking 2 = 60 ms).
"""
from .config import FRAME_SECONDS, LABELS

SPACE = LABELS.index(" ")


def word_timings(tokens, frames, conf=None):
    """One utterance's tokens (label ids), their emission frames and (optionally) confidences, each
    trimmed to the utterance's res_len -> [(word, start_s, end_s, min_conf)].

    Words are the runs of non-space labels (leading, trailing and repeated spaces give no empty
    words); start_s is the start of the first token's frame, end_s the end of the last token's frame,
    min_conf the smallest confidence over the word's tokens (None without conf)."""
    tokens = [int(t) for t in tokens]
    frames = [int(f) for f in frames]
    conf = None if conf is None else [float(c) for c in conf]
    if len(frames) != len(tokens) or (conf is not None and len(conf) != len(tokens)):
        raise ValueError("tokens, frames and conf must have the same length (trim them to res_len)")
    words, first = [], None
    for i in range(len(tokens) + 1):
        if i < len(tokens) and tokens[i] != SPACE:
            if not 0 <= tokens[i] < len(LABELS):
                raise ValueError(f"token {tokens[i]} at {i} is not a label (trim the row to res_len)")
            if first is None:
                first = i
            continue
        if first is not None:
            word = "".join(LABELS[t] for t in tokens[first:i])
            words.append((word, frames[first] * FRAME_SECONDS, (frames[i - 1] + 1) * FRAME_SECONDS,
                          None if conf is None else min(conf[first:i])))
            first = None
    return words
