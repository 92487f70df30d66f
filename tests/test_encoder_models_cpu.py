"""Synthetic encoder models (tests/encoder_models.py), CPU side: the .drmenc writer against the oracle's reader and the
product's exporter, the loader's refusals (drm_encoder_export is host only), and the conditions that keep
tests/test_gpu_encoder_models.py honest -- each is a property of the models and of the oracle, measured here and never
on the GPU: the bar is no wider than four times the shipped model's, both "lost lo term" mutants of the oracle miss it by
a factor of three, and every model reaches the edge it was made for."""
import os
import struct

import numpy as np
import pytest

import encoder_models as EM
from oracle import gru_oracle as G


def _export_code(src, tmp_path):
    from deepreadmapper_amd import export_encoder
    from deepreadmapper_amd._native import DrmError
    with pytest.raises(DrmError) as e:
        export_encoder(src, tmp_path / "refused.drmenc")
    assert not os.path.exists(tmp_path / "refused.drmenc")
    return e.value.code


# ------------------------------------------------------------------------------------- writer
@pytest.mark.parametrize("name", EM.MODELS)
def test_writer_round_trip(name, tmp_path):
    from deepreadmapper_amd import export_encoder
    w = EM.model(name)
    path = EM.write_drmenc(tmp_path / f"{name}.drmenc", w)
    back = G.load_drmenc(path)
    assert sorted(back) == sorted(w)
    assert back["h0"] == w["h0"] and np.array_equal(back["vocab_rows"], w["vocab_rows"])
    for k in EM.TENSORS:
        assert back[k].shape == w[k].shape and np.array_equal(back[k], w[k]), k
    export_encoder(path, tmp_path / "exported.drmenc")        # the product's reader and writer agree with ours
    assert open(tmp_path / "exported.drmenc", "rb").read() == open(path, "rb").read()


def test_writer_reproduces_shipped_file(tmp_path):
    path = EM.write_drmenc(tmp_path / "shipped.drmenc", G.load_drmenc(EM.SHIPPED))
    assert open(path, "rb").read() == open(EM.SHIPPED, "rb").read()


def test_writer_refuses_inexact_values(tmp_path):
    w = dict(EM.model("h0pos"))
    with pytest.raises(AssertionError):
        EM.write_drmenc(tmp_path / "a.drmenc", dict(w, h0=0.3))                   # 0.3 is no f32 number
    with pytest.raises(AssertionError):
        EM.write_drmenc(tmp_path / "b.drmenc", dict(w, B1=w["B1"] + 2.0 ** -30))    # nor this an f16 tensor


# ------------------------------------------------------------------------------------- loader refusals
@pytest.fixture(scope="module")
def good_bytes(tmp_path_factory):
    path = EM.write_drmenc(tmp_path_factory.mktemp("enc") / "good.drmenc", EM.model("h0pos"))
    return open(path, "rb").read()


def _patched(b, offset, fmt, value):
    return b[:offset] + struct.pack(fmt, value) + b[offset + struct.calcsize(fmt):]


def test_loader_accepts_the_unpatched_file(good_bytes, tmp_path):
    from deepreadmapper_amd import export_encoder
    (tmp_path / "good.drmenc").write_bytes(good_bytes)
    export_encoder(tmp_path / "good.drmenc", tmp_path / "out.drmenc")
    assert (tmp_path / "out.drmenc").read_bytes() == good_bytes


def test_loader_refuses_other_hidden_size(good_bytes, tmp_path):
    from deepreadmapper_amd._native import DRM_ERR_UNSUPPORTED
    assert struct.unpack_from("<I", good_bytes, 12)[0] == 64        # header word 1 = hidden
    (tmp_path / "h32.drmenc").write_bytes(_patched(good_bytes, 12, "<I", 32))
    assert _export_code(tmp_path / "h32.drmenc", tmp_path) == DRM_ERR_UNSUPPORTED


def test_loader_refuses_other_token_table(good_bytes, tmp_path):
    from deepreadmapper_amd._native import DRM_ERR_UNSUPPORTED
    off = 36 + 2 * 40                                                # vocabulary id of row 40
    row = struct.unpack_from("<H", good_bytes, off)[0]
    assert row == EM.model("h0pos")["vocab_rows"][40]
    (tmp_path / "vocab.drmenc").write_bytes(_patched(good_bytes, off, "<H", row + 1))
    assert _export_code(tmp_path / "vocab.drmenc", tmp_path) == DRM_ERR_UNSUPPORTED


def test_loader_refuses_trailing_byte(good_bytes, tmp_path):
    from deepreadmapper_amd._native import DRM_ERR_FORMAT
    (tmp_path / "tail.drmenc").write_bytes(good_bytes + b"\0")
    assert _export_code(tmp_path / "tail.drmenc", tmp_path) == DRM_ERR_FORMAT


@pytest.mark.parametrize("nrows", [98, 105, 100_000, 1 << 22])
def test_loader_refuses_rows_past_the_end(good_bytes, tmp_path, nrows):
    """98 runs out in the last tensor, 105 moves the 16-byte pad, 100,000 runs out in the embedding rows and 2^22 in the
    token table itself."""
    from deepreadmapper_amd._native import DRM_ERR_FORMAT
    assert struct.unpack_from("<I", good_bytes, 24)[0] == 97        # header word 4 = rows
    (tmp_path / "rows.drmenc").write_bytes(_patched(good_bytes, 24, "<I", nrows))
    assert _export_code(tmp_path / "rows.drmenc", tmp_path) == DRM_ERR_FORMAT


# ------------------------------------------------------------------------------------- oracle hooks
def test_oracle_hooks_default_to_the_float64_oracle():
    """The hooks the variants use change nothing while unused, and an identity hook changes nothing either."""
    w, tok = EM.model("shipped"), EM.tokens()[:5]
    ref = G.encode_tokens(w, tok)
    assert ref.dtype == np.float64
    same = G.encode_tokens(w, tok, dtype=np.float64, round_h=lambda h: h, round_y1=lambda y: y,
                           probe=lambda layer, z, r, n: None)
    assert np.array_equal(ref, same)
    assert np.array_equal(ref, G.vectorize(w, list(EM.reads()[:5])))
    assert G.encode_tokens(w, tok, dtype=np.float32).dtype == np.float32


# ------------------------------------------------------------------------------------- conditions of the GPU bars
def test_reads_are_two_tiles_and_a_partial_one():
    assert len(EM.reads()) == 70 and EM.tokens().shape == (70, G.MAX_LEN)
    assert all(len(r) >= 2 for r in EM.reads())


@pytest.mark.parametrize("name", EM.MODELS)
def test_bar_is_close_to_the_shipped_models(name):
    ratio = EM.e32(name) / EM.e32("shipped")
    print(f"{name}: e32 {EM.e32(name):.3g}, shipped {EM.e32('shipped'):.3g}, ratio {ratio:.3g}, tol {EM.tol(name):.3g}")
    assert EM.e32("shipped") > 0 and 0 < ratio <= 4
    assert np.isfinite(EM.reference(name)).all()


@pytest.mark.parametrize("name", EM.MODELS)
def test_lost_lo_terms_miss_the_bar(name):
    w, ref = EM.model(name), EM.reference(name)
    dh = np.abs(EM.mutant_state_hi_only(w) - ref).max()
    dy = np.abs(EM.mutant_y1_hi_only(w) - ref).max()
    print(f"{name}: state hi only moves {dh:.3g}, layer-1 output hi only {dy:.3g}, tol {EM.tol(name):.3g}")
    assert dh >= 3 * EM.tol(name) and dy >= 3 * EM.tol(name)


@pytest.mark.parametrize("name", ["h0pos", "h0neg", "pinned"])
def test_h0_models_depend_on_h0(name):
    w = EM.model(name)
    h0hi = float(np.float16(w["h0"]))
    assert w["h0"] != 0 and w["h0"] != h0hi                          # the seeded state has a lo half
    moved = np.abs(EM.oracle64(dict(w, h0=0.0)) - EM.reference(name)).max()
    print(f"{name}: h0 -> 0 moves {moved:.3g}")
    assert moved > 0.1


def test_hot_sees_a_seed_without_its_lo_half():
    """h0 = 0.7 lies 2e-4 from its f16 rounding and `hot` hardly damps it; 0.3 and -0.77 lie 4.9e-5 and 2e-5 away,
    which the other models' recurrences contract below the bar."""
    w = EM.model("hot")
    assert abs(w["h0"] - float(np.float16(w["h0"]))) > 1.9e-4
    lost = np.abs(EM.mutant_seed_hi_only(w) - EM.reference("hot")).max()
    print(f"hot: seed hi only moves {lost:.3g}")
    assert lost >= 3 * EM.tol("hot")


def test_pinned_reaches_the_saturated_gates():
    ext = {}

    def probe(layer, z, r, n):
        for g, a in zip("zrn", (z, r, n)):
            lo, hi = ext.get((layer, g), (0.0, 0.0))
            ext[(layer, g)] = (min(lo, float(a.min())), max(hi, float(a.max())))

    w = EM.model("pinned")
    out = EM.oracle64(w, probe=probe)
    assert np.array_equal(out, EM.reference("pinned")) and np.isfinite(out).all()
    assert sorted(ext) == [(layer, g) for layer in (1, 2) for g in "nrz"]
    for key, (lo, hi) in ext.items():                                 # float32 exp() leaves its range at +-88.7
        assert lo < -88.8 and hi > 88.8, (key, lo, hi)
    # z == 1 carries h0 through all 123 steps of both layers, in float64 and in float32
    cols = [d * EM.H + j for d in range(2) for j in range(EM.H) if j % 8 == EM.PIN_Z1]
    assert len(cols) == 16 and (out[:, cols] == w["h0"]).all()
    assert (EM.oracle32(w)[:, cols] == w["h0"]).all()
    others = [c for c in range(2 * EM.H) if c not in cols]
    assert (np.abs(out[:, others] - w["h0"]) > 1e-3).mean() > 0.9


def test_subnormal_w1_is_subnormal():
    w = EM.model("subnormal_w1")
    a = np.abs(w["W1"])
    assert (a > 0).all() and (a < 2.0 ** -14).all()
    bits = w["W1"].astype(np.float16).view(np.uint16)
    assert ((bits & 0x7C00) == 0).all() and ((bits & 0x03FF) != 0).all()   # exponent field 0, mantissa not
    assert len(np.unique(bits)) > 1000 and (a == EM.F16_MAX_SUB).mean() < 1e-3
    assert w["h0"] == 0.0
    flushed = np.abs(EM.oracle64(dict(w, W1=np.zeros_like(w["W1"]))) - EM.reference("subnormal_w1")).max()
    print(f"subnormal_w1: W1 flushed to zero moves {flushed:.3g}")
    assert flushed > 0.1
