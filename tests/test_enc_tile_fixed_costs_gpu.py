"""The tick tile's staged fixed inputs (encoder.hip): the sigma table, the tile's bias floats and the
StackTime row lengths reach LDS by DMA with the cell state, and the epilogue and the copy-out read
them there.  Every case runs the int8 encoder against the CPU restatement and requires bit equality,
at the smallest shapes at which that staging can go wrong: a last batch tile that is mostly
padding, odd lengths mixed within one tile (the zero pad frame and the past-length masking both
read the staged lengths), ticks with fewer active tiles than the first, and two encodes back to
back on different tiles.  The synthetic model's biases are non-zero (checked)."""
import numpy as np
import pytest

from rnnt_amd import synthetic, weights
from rnnt_amd.engine import pad_batch

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

T = 5


@pytest.fixture(scope="module")
def model():
    pm, _ = weights.build_model()
    assert all(np.count_nonzero(b) > b.size // 2 for b in pm.enc_bq), "the cases need a non-zero bias"
    return pm


@pytest.fixture(scope="module")
def engine(model):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from rnnt_amd.engine import Engine
    e = Engine(model, device=0, max_batch=512, max_frames=32)
    yield e
    e.set_tile("auto")
    e.close()


def _lens(n):
    """{5, 4, 1, 3, 2} mixed within the first 128-row tile; the rows of every later 128-row tile
    are shorter (3, 1, ...), so the ticks of frames >= 4 run fewer batch tiles than the first."""
    lens = np.array([5, 4, 1, 3, 2], np.int32)[np.arange(n) % 5]
    lens[128:] = np.array([3, 1], np.int32)[np.arange(n - 128) % 2] if n > 128 else lens[128:]
    if n > 256:
        lens[256:] = 1
    return lens


@pytest.fixture(scope="module")
def cases(model, oracle):
    """(features, lengths, oracle frames) per batch size, computed once"""
    out = {}
    for n, seed in ((128, 21), (130, 22), (257, 23)):
        lens = _lens(n)
        x = synthetic.make_features(T, n, seed=seed, lens=lens)
        out[n] = (x, lens, oracle.encoder_i8(model, x, lens))
    return out


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _encode_check(engine, case, tag):
    x, lens, fo = case
    n = len(lens)
    n_pad = pad_batch(n)
    xp = np.zeros((T, n_pad, x.shape[2]), np.float32)
    xp[:, :n] = x
    lp = np.zeros(n_pad, np.int32)
    lp[:n] = lens
    f = torch.zeros(((T + 1) // 2, n_pad, 1024), dtype=torch.float32, device="cuda")
    engine.encode(_cuda(xp), _cuda(lp), lens, n=n, f_out=f)
    torch.cuda.synchronize()
    fg = f.cpu().numpy()
    for i in range(n):
        fl = (int(lens[i]) + 1) // 2
        assert np.array_equal(fg[:fl, i].view(np.uint32), fo[:fl, i].view(np.uint32)), f"{tag}: row {i} (length {lens[i]})"


@pytest.mark.parametrize("tile,n", [("big", 130), ("big", 257), ("small", 130), ("tiny", 130), ("mini", 130)])
def test_padded_last_tile_mixed_lengths(engine, cases, tile, n):
    """N = 130 / 257: the last batch tile holds 2 / 1 live rows and padding; lengths {5, 4, 1, ..}
    in one tile, T odd."""
    engine.set_tile(tile)
    _encode_check(engine, cases[n], f"{tile} N={n}")


def test_back_to_back_encodes_on_different_tiles(engine, cases):
    """Two encodes in a row on one engine, different tiles and inputs: the LDS images a previous
    workgroup left on a CU (table, bias, lengths) belong to another tile shape and batch."""
    engine.set_tile("big")
    _encode_check(engine, cases[257], "big N=257 first")
    engine.set_tile("mini")
    _encode_check(engine, cases[130], "mini N=130 second")
    engine.set_tile("big")
    _encode_check(engine, cases[130], "big N=130 third")


def test_flow_path_shares_the_step(engine, cases):
    """the persistent dataflow launch runs the same step body (bias and lengths staged per task)"""
    engine.set_tile("flow")
    _encode_check(engine, cases[128], "flow N=128")


@pytest.fixture(scope="module")
def chunk(model, oracle):
    """One Server chunk of 256 slots whose FIRST 128-row tile finishes long before the second, with
    the oracle's tokens; 24 frames, because shorter chunks emit nothing on this model."""
    n, Tc = 256, 24
    lens = np.concatenate([np.array([3, 1, 2], np.int32)[np.arange(128) % 3], np.full(128, 2, np.int32)])
    lens[128:160] = np.array([24, 23, 19, 21], np.int32)[np.arange(32) % 4]
    x = synthetic.make_features(Tc, n, seed=24, lens=lens)
    fo = oracle.encoder_i8(model, x, lens)
    ro, rlo, _ = oracle.greedy_decode(model, fo, (lens + 1) // 2, max_res=Tc * 30)
    assert int(rlo[128:].sum()) > 0, "the chunk emits nothing"
    return Tc, lens, x, ro, rlo


@pytest.mark.parametrize("tile", ["big", "small"])
def test_stream_chunk_skips_inner_tiles(engine, chunk, tile):
    """The tick's tile mask (a set of active tiles, not a leading count): the stream path returns no
    frames, so the tokens of its decode are compared with the greedy decode of the oracle's frames."""
    Tc, lens, x, ro, rlo = chunk
    n = len(lens)
    off = np.concatenate([[0], np.cumsum(lens[:-1])]).astype(np.int64)
    store = _cuda(np.concatenate([x[: lens[i], i, :240] for i in range(n)]))
    reset = torch.ones(n, dtype=torch.int32, device="cuda")
    res = torch.zeros((n, engine.max_res), dtype=torch.int32, device="cuda")
    rl = torch.zeros(n, dtype=torch.int32, device="cuda")
    engine.set_tile(tile)
    engine.encode_stream(store, _cuda(off), _cuda(lens), lens, reset, Tc, n, n)
    engine.decode_stream(res, rl, reset)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(rl.cpu().numpy(), rlo)
    rg = res.cpu().numpy()
    for i in range(n):
        np.testing.assert_array_equal(rg[i, : rlo[i]], ro[i, : rlo[i]], err_msg=f"tokens, slot {i}")
