"""TEST INFRASTRUCTURE ONLY -- synthetic read-encoder models and the bars to hold the GPU encoder to on them.

The shipped weights leave most of csrc/encoder_gru.hip's arithmetic edges unreached (h0 = 0, no pre-activation past
+-13.6, no zero or subnormal weight). The models here reach them. All are deterministic from fixed seeds, carry the real
token table (the loader refuses any other), have every tensor rounded to f16 and h0 to f32, and are written to disk by
write_drmenc below, which follows the layout oracle.gru_oracle.load_drmenc reads.

Common base: W ~ N(0, sw / sqrt(in)), R ~ N(0, sr / sqrt(64)), B ~ N(0, sb), embedding rows ~ N(0, 1).
  h0pos          sw 1.0, sr 0.8, sb 0.3, h0 = 0.3 (not an f16 number: the lo half of the seeded state is non-zero)
  h0neg          the same base from another seed, h0 = -0.77
  pinned         the base with h0 = 0.3 and, in every layer and direction, by unit j % 8:
                   0: b_z = +120 (z == 1: the unit carries h0 through every step)    1: b_z = -120 (z == 0)
                   2: b_r = -120 (r == 0)         3: b_r = +120 (r == 1)
                   4: Wb_n = +100 (tanh == 1)     5: Rb_n = -100
                   6: Wb_n = +65504 forward, -65504 backward (the largest f16)        7: untouched
                 exp() of the float32 gate math overflows to inf and underflows to 0 on these units
  subnormal_w1   the base with h0 = 0, embedding rows x 2^12 and W1 x 2^-13: every W1 entry an f16 subnormal (a zero after
                 rounding becomes the smallest one, the few beyond the largest are clipped to it), products x W of O(1)
  hot            sw 2.0, sr 2.0, sb 0.5, h0 = 0.7: a less contractive recurrence than the trained model's

The bar of a model comes from the oracle alone, never from the GPU:
  e32(model) = max |float32 oracle - float64 oracle| on the test reads,
  tol(model) = ENC_ATOL * max(1, e32(model) / e32(shipped)),
so every model gets the headroom over plain f32 arithmetic that the shipped model's ENC_ATOL has. Two mutants of the
oracle lose what the kernel's hi/lo split carries: the state rounded to f16 before the recurrent product, and layer 1's
output rounded to f16 before layer 2 (tests/test_encoder_models_cpu.py requires both to miss every model's bar). A third
loses the lo half of the seeded state alone; `hot` is the model that has to see it."""
import functools
import os
import struct

import numpy as np

from oracle import gru_oracle as G
from test_gpu_encoder import ENC_ATOL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SHIPPED = os.path.join(ROOT, "deepreadmapper_amd", "models", "finetuned_sgn33-new-a-Apr6.drmenc")
N_READS = 70          # two full tiles of 32 and a partial one
H = G.HIDDEN
TENSORS = ("emb_rows", "W1", "R1", "B1", "W2", "R2", "B2")
F16_MIN_SUB, F16_MAX_SUB = 2.0 ** -24, 1023 * 2.0 ** -24
PIN_Z1, PIN_Z0 = 0, 1  # unit j % 8 of `pinned` with z == 1, z == 0


# ------------------------------------------------------------------------------------- the file
def write_drmenc(path, w):
    """w (the dict load_drmenc returns) -> .drmenc: magic, 7 x u32 (version 1, hidden, emb dim, max len, rows, layers 2,
    0), the rows' vocabulary ids u16, zero pad to 16 bytes, h0 as 4 x f32 (h0, 0, 0, 0), the embedding rows f16, then
    W, R, B f16 per layer. Refuses a value that the file's f16 / f32 would not hold exactly."""
    def f16(a, shape):
        a = np.asarray(a, dtype=np.float64)
        assert a.shape == shape, (a.shape, shape)
        with np.errstate(over="raise"):
            b = a.astype("<f2")
        assert np.array_equal(b.astype(np.float64), a), "tensor is not f16-exact"
        return b.tobytes()

    vocab = np.asarray(w["vocab_rows"])
    nrows = len(vocab)
    edim = np.asarray(w["emb_rows"]).shape[1]
    assert float(np.float32(w["h0"])) == w["h0"], "h0 is not an f32 number"
    out = b"DRMENC1\0" + struct.pack("<7I", 1, H, edim, G.MAX_LEN, nrows, 2, 0)
    out += vocab.astype("<u2").tobytes()
    out += b"\0" * (-len(out) % 16)
    out += struct.pack("<4f", w["h0"], 0.0, 0.0, 0.0)
    out += f16(w["emb_rows"], (nrows, edim))
    for li, ind in enumerate((edim, 2 * H)):
        out += f16(w[f"W{li + 1}"], (2, 3 * H, ind))
        out += f16(w[f"R{li + 1}"], (2, 3 * H, H))
        out += f16(w[f"B{li + 1}"], (2, 4 * H))
    with open(path, "wb") as f:
        f.write(out)
    return path


# ------------------------------------------------------------------------------------- the models
def _f16(a):
    return np.asarray(a).astype(np.float16).astype(np.float64)


def _vocab_rows():
    return np.concatenate([[0], G.tok2index()]).astype(np.int64)


def _base(seed, sw, sr, sb, h0):
    rng = np.random.default_rng(seed)
    w = {"vocab_rows": _vocab_rows(), "h0": float(np.float32(h0))}
    w["emb_rows"] = _f16(rng.normal(0.0, 1.0, (1 + 96, 64)))
    for li, ind in enumerate((64, 2 * H)):
        w[f"W{li + 1}"] = _f16(rng.normal(0.0, sw / np.sqrt(ind), (2, 3 * H, ind)))
        w[f"R{li + 1}"] = _f16(rng.normal(0.0, sr / np.sqrt(H), (2, 3 * H, H)))
        w[f"B{li + 1}"] = _f16(rng.normal(0.0, sb, (2, 4 * H)))
    return w


def _pinned():
    w = _base(103, 1.0, 0.8, 0.3, 0.3)
    j = np.arange(H)
    for li in (1, 2):
        B = w[f"B{li}"]
        for d in range(2):
            B[d, 0 * H + j[j % 8 == 0]] = 120.0     # b_z
            B[d, 0 * H + j[j % 8 == 1]] = -120.0
            B[d, 1 * H + j[j % 8 == 2]] = -120.0    # b_r
            B[d, 1 * H + j[j % 8 == 3]] = 120.0
            B[d, 2 * H + j[j % 8 == 4]] = 100.0     # Wb_n
            B[d, 3 * H + j[j % 8 == 5]] = -100.0    # Rb_n
            B[d, 2 * H + j[j % 8 == 6]] = -65504.0 if d else 65504.0
    return w


def _subnormal_w1():
    w = _base(104, 1.0, 0.8, 0.3, 0.0)
    w["emb_rows"] = _f16(w["emb_rows"] * 2.0 ** 12)
    w1 = _f16(w["W1"] * 2.0 ** -13)
    w["W1"] = np.where(w["W1"] < 0, -1.0, 1.0) * np.clip(np.abs(w1), F16_MIN_SUB, F16_MAX_SUB)
    return w


_RECIPES = {
    "h0pos": lambda: _base(101, 1.0, 0.8, 0.3, 0.3),
    "h0neg": lambda: _base(102, 1.0, 0.8, 0.3, -0.77),
    "pinned": _pinned,
    "subnormal_w1": _subnormal_w1,
    "hot": lambda: _base(105, 2.0, 2.0, 0.5, 0.7),
}
MODELS = tuple(_RECIPES)
H0_MODELS = ("h0pos", "h0neg", "pinned", "hot")


@functools.lru_cache(maxsize=None)
def model(name):
    """The weights of one model (shared: treat as read-only); "shipped" = the trained model."""
    return G.load_drmenc(SHIPPED) if name == "shipped" else _RECIPES[name]()


# ------------------------------------------------------------------------------------- the oracle's variants
@functools.lru_cache(maxsize=None)
def reads():
    from conftest import read_fastq_tagged
    return tuple(read_fastq_tagged(os.path.join(GOLDEN, "test_data.fastq"))[:N_READS])


@functools.lru_cache(maxsize=None)
def tokens():
    return G.model_input(list(reads()))


def _to_f16(dtype):
    return lambda a: a.astype(np.float16).astype(dtype)


def oracle64(w, tok=None, probe=None):
    """The project's oracle: float64 on the f16-exact weights."""
    return G.encode_tokens(w, tokens() if tok is None else tok, probe=probe)


def oracle32(w, tok=None):
    """The same formulas in plain float32: what f32 gate math costs with nothing else lost."""
    return G.encode_tokens(w, tokens() if tok is None else tok, dtype=np.float32).astype(np.float64)


def mutant_state_hi_only(w, tok=None):
    """The state enters the recurrent product as its f16 rounding alone (the kernel's lo term lost)."""
    return G.encode_tokens(w, tokens() if tok is None else tok, round_h=_to_f16(np.float64))


def mutant_y1_hi_only(w, tok=None):
    """Layer 1's output enters layer 2 as its f16 rounding alone (the lo half of the layer-1 rows lost)."""
    return G.encode_tokens(w, tokens() if tok is None else tok, round_y1=_to_f16(np.float64))


def mutant_seed_hi_only(w, tok=None):
    """The first recurrent product of each layer sees f16(h0) alone (the lo half of the seeded state image lost, the
    carried f32 state right): what tells is a large h0 - f16(h0) under a recurrence that does not damp it, i.e. `hot`."""
    h0 = w["h0"]
    return G.encode_tokens(w, tokens() if tok is None else tok,
                           round_h=lambda h: _to_f16(np.float64)(h) if (h == h0).all() else h)


@functools.lru_cache(maxsize=None)
def reference(name):
    """float64 oracle of the test reads, computed once per model (read-only)."""
    r = oracle64(model(name))
    r.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def e32(name):
    return float(np.abs(oracle32(model(name)) - reference(name)).max())


def tol(name):
    return ENC_ATOL * max(1.0, e32(name) / e32("shipped"))
