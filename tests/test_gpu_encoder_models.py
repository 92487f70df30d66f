"""Read encoder on the GPU, on the paths the shipped weights cannot reach (tests/encoder_models.py has the models and the
rule for their bars; tests/test_encoder_models_cpu.py shows that the bars bite). Reads: the first 70 of C1, two full
tiles and a partial one.

* every synthetic model: h0 arrives from the file, max |gpu - float64 oracle| <= tol(model); `pinned` (exp() overflowing
  and underflowing, z, r exactly 0 and 1, tanh exactly +-1) stays finite and its z == 1 units carry h0 to the output;
* two encoders with different models alive at once do not disturb each other;
* the device entry point encodes rows shorter than 2 as padding and counts them, counts undefined tokens once (not once
  per direction), and drm_encoder_flags resets on read;
* no byte at or past lens[i] is read: tokens and embeddings do not depend on what lies there;
* a read's embedding does not depend on the batch size around the tile edges (n = 1, 31, 32, 33, 64, 65), on the tiles
  per launch, or on how often the handle's layer-1 workspace has grown; the workspace grows by whole tiles and only grows.

Measured on the MI355X (max |gpu - oracle| over 70 x 128 outputs; e32 = the float32 oracle's own distance; every
tol(model) is ENC_ATOL = 2e-5, no model's e32 exceeding the shipped model's 1.36e-6):
  model          gpu error   e32        gpu / e32
  h0pos          2.48e-07    3.51e-07   0.71
  h0neg          2.80e-07    2.93e-07   0.96
  pinned         5.36e-07    5.94e-07   0.90
  subnormal_w1   2.31e-07    2.43e-07   0.95     (the matrix unit keeps f16 subnormal operands: no refusal needed)
  hot            7.86e-07    1.27e-06   0.62
pinned's largest error is on its z == 1 units: they end 5.4e-7 from h0 where both oracles end on h0 exactly, because
the kernel's h' = n + z (h - n) rounds h - n and the sum again at z == 1 (half an ulp of |h - n| <= 2 per step, not
contracted by anything while z == 1), where (1 - z) n + z h returns h. Short rows: 1.9e-6 (shipped) and 1.8e-7 (h0neg)
from the oracle's all-padding embedding.
"""
import os

import numpy as np
import pytest

import encoder_models as EM
from oracle import gru_oracle as G

pytestmark = pytest.mark.gpu

TILE_BYTES = 123 * 32 * 256 * 2   # layer-1 output of one tile of 32 reads: hi and lo f16 of 2 x 64 units per step


@pytest.fixture(scope="module")
def paths(tmp_path_factory):
    d = tmp_path_factory.mktemp("encoder_models")
    return {name: str(EM.write_drmenc(d / f"{name}.drmenc", EM.model(name))) for name in EM.MODELS}


@pytest.fixture(scope="module")
def solo(paths):
    """name -> embeddings of the test reads from an encoder that was alone on the GPU (computed once, read-only)."""
    from deepreadmapper_amd import Encoder
    cache = {}

    def get(name):
        if name not in cache:
            e = Encoder(paths[name])
            try:
                cache[name] = e.vectorize(list(EM.reads()))
            finally:
                e.free()
            cache[name].setflags(write=False)
        return cache[name]
    return get


@pytest.fixture(scope="module")
def enc():
    from deepreadmapper_amd import Encoder
    e = Encoder()
    yield e
    e.free()


# ------------------------------------------------------------------------------------- the models
@pytest.mark.parametrize("name", EM.MODELS)
def test_model_vs_oracle(name, paths, solo):
    from deepreadmapper_amd import Encoder
    w = EM.model(name)
    e = Encoder(paths[name])
    try:
        assert e.info.h0 == np.float32(w["h0"])
    finally:
        e.free()
    got, ref, tol = solo(name), EM.reference(name), EM.tol(name)
    assert got.shape == ref.shape == (EM.N_READS, 128) and got.dtype == np.float32
    err = np.abs(got.astype(np.float64) - ref)
    print(f"{name}: max abs err {err.max():.3g}, mean {err.mean():.3g}; e32 {EM.e32(name):.3g}, "
          f"err / e32 {err.max() / EM.e32(name):.3g}, tol {tol:.3g}")
    assert np.isfinite(got).all()
    assert err.max() <= tol


def test_pinned_z1_units_carry_h0(solo):
    w = EM.model("pinned")
    got = solo("pinned")
    cols = [d * EM.H + j for d in range(2) for j in range(EM.H) if j % 8 == EM.PIN_Z1]
    dev = np.abs(got[:, cols].astype(np.float64) - w["h0"])
    print(f"pinned: z == 1 units end {dev.max():.3g} from h0")
    assert np.isfinite(got).all()
    assert dev.max() <= EM.tol("pinned")


def test_two_models_alive_at_once(paths, solo):
    from deepreadmapper_amd import Encoder
    names = ("h0pos", "pinned", "hot")
    encs = [Encoder(paths[n]) for n in names]
    try:
        for _ in range(2):                       # interleaved, so each handle's workspace is reused after the others ran
            for n, e in zip(names, encs):
                assert e.info.h0 == np.float32(EM.model(n)["h0"])
                assert np.array_equal(e.vectorize(list(EM.reads())), solo(n)), n
    finally:
        for e in encs:
            e.free()


# ------------------------------------------------------------------------------------- device entry, short rows
_SHORT_AT = {0: 1, 5: 0, 31: -5, 32: 1, 47: 0}   # row -> its length: first, inside, both sides of a tile edge, last


def _with_short_rows(valid):
    """(buf, lens, rows of the valid reads) with short rows put among `valid`; a short row's bytes are bases, not zeros."""
    n = len(valid) + len(_SHORT_AT)
    assert max(_SHORT_AT) == n - 1
    stride = max(len(s) for s in valid)
    buf = np.zeros((n, stride), np.uint8)
    lens = np.zeros(n, np.int32)
    it, rows = iter(valid), []
    for i in range(n):
        if i in _SHORT_AT:
            buf[i] = np.frombuffer((b"ACGT" * stride)[:stride], np.uint8)
            lens[i] = _SHORT_AT[i]
        else:
            s = next(it)
            buf[i, :len(s)] = np.frombuffer(s, np.uint8)
            lens[i] = len(s)
            rows.append(i)
    return buf, lens, np.array(rows)


@pytest.mark.parametrize("name", ["shipped", "h0neg"])
def test_device_entry_short_rows(name, paths):
    from deepreadmapper_amd import Encoder
    from deepreadmapper_amd.device import DeviceBuffer, Stream
    w = EM.model(name)
    valid = list(EM.reads()[:40]) + [b"<ACGTNNACGTACGNTT>", b"NN", b"<" + b"ACGNT" * 30 + b">"]
    und = int((G.model_input(valid) == -1).sum())
    assert und > 3
    buf, lens, rows = _with_short_rows(valid)
    short = np.array(sorted(_SHORT_AT))
    e = Encoder(paths[name]) if name != "shipped" else Encoder()
    try:
        want, und_host = e.vectorize(valid, return_undefined=True)
        assert und_host == und
        d_s, d_l = DeviceBuffer.from_host(buf), DeviceBuffer.from_host(lens)
        d_o = DeviceBuffer((len(lens), 128), np.float32)
        st = Stream()
        d_o.upload(np.full((len(lens), 128), np.nan, np.float32))
        e.vectorize_device(d_s, d_l, len(lens), buf.shape[1], d_o, st)
        st.synchronize()
        got = d_o.download()
        assert np.array_equal(got[rows], want)
        pad = G.encode_tokens(w, np.zeros((1, G.MAX_LEN), np.int64))[0]
        err = np.abs(got[short].astype(np.float64) - pad).max()
        print(f"{name}: short rows {err:.3g} from the oracle's all-padding embedding")
        assert err <= EM.tol(name)
        assert (got[short] == got[short[0]]).all()
        e.vectorize_device(d_s, d_l, len(lens), buf.shape[1], d_o, st)
        st.synchronize()
        assert np.array_equal(d_o.download(), got)
        assert e.flags() == (2 * und, 2 * len(short))
        assert e.flags() == (0, 0)
        for b in (d_s, d_l, d_o):
            b.free()
    finally:
        e.free()


# ------------------------------------------------------------------------------------- bytes past the end
def _ragged_batch(stride=200, seed=7):
    rng = np.random.default_rng(seed)
    lens = np.concatenate([[2, 3, 121, 122, 123, 124, 125, 199, 200], rng.integers(2, 201, size=91)]).astype(np.int32)
    alpha = np.frombuffer(b"ACGTacgtN<>", dtype=np.uint8)
    buf = alpha[rng.integers(0, len(alpha), size=(len(lens), stride))]
    return np.ascontiguousarray(buf), lens


def test_bytes_past_the_end_are_not_read(enc):
    buf, lens = _ragged_batch()
    past = np.arange(buf.shape[1])[None, :] >= lens[:, None]
    assert past.sum() > 5000 and not past[8].any()          # row 8 fills its stride
    zero = np.where(past, 0, buf).astype(np.uint8)
    tok0, vec0 = enc.tokenize((zero, lens)), enc.vectorize((zero, lens))
    assert np.array_equal(tok0, G.model_input([bytes(zero[i, :lens[i]]) for i in range(len(lens))]))
    for fill in (0xFF, ord("<"), ord(">"), ord("A")):
        filled = np.where(past, fill, buf).astype(np.uint8)
        assert np.array_equal(enc.tokenize((filled, lens)), tok0), hex(fill)
        assert np.array_equal(enc.vectorize((filled, lens)), vec0), hex(fill)


# ------------------------------------------------------------------------------------- tile edges, workspace
_EDGE_N = (1, 31, 32, 33, 64, 65)


@pytest.mark.parametrize("tiles", [None, "1", "2"])
def test_prefix_batches_at_tile_edges(tiles, enc):
    from deepreadmapper_amd import Encoder
    seqs = list(EM.reads()[:65])
    full = enc.vectorize(seqs)
    old = os.environ.get("DRM_ENC_TILES")
    try:
        if tiles is None:
            os.environ.pop("DRM_ENC_TILES", None)
        else:
            os.environ["DRM_ENC_TILES"] = tiles
        e = Encoder()
    finally:
        if old is None:
            os.environ.pop("DRM_ENC_TILES", None)
        else:
            os.environ["DRM_ENC_TILES"] = old
    try:
        for n in _EDGE_N:
            assert np.array_equal(e.vectorize(seqs[:n]), full[:n]), n
        assert e.info.device_bytes - _weights_bytes(e) == (3 if tiles is None else int(tiles)) * TILE_BYTES
    finally:
        e.free()


def _weights_bytes(e):
    """device_bytes of the handle's weights alone: what a fresh handle of the same model reports."""
    from deepreadmapper_amd import Encoder
    f = Encoder(e.path)
    try:
        return f.info.device_bytes
    finally:
        f.free()


def test_workspace_grows_by_tiles_and_never_shrinks(enc):
    from deepreadmapper_amd import Encoder
    seqs = list(EM.reads()[:65])
    full = enc.vectorize(seqs)
    e = Encoder()
    try:
        base = e.info.device_bytes
        seen = [base]
        for n, tiles in ((33, 2), (1, 2), (65, 3), (33, 3)):
            assert np.array_equal(e.vectorize(seqs[:n]), full[:n]), n
            seen.append(e.info.device_bytes)
            assert seen[-1] == base + tiles * TILE_BYTES, (n, seen)
        assert seen == sorted(seen)
        assert seen[3] - seen[2] == TILE_BYTES
    finally:
        e.free()
