"""GPU tests of drm_bgzf_compress (csrc/bgzf.hip): every stream goes through the independent reader of tests/bam_ref.py
(every header byte, BSIZE, each member inflated alone by zlib, CRC-32, ISIZE) and must inflate to the input. Where a case
says which form a member has, or how small it must be, that is asserted too: a kernel that stored everything would pass
nothing else here. Sizes: the block edges; runs; every match length; the distance limit; matches cut at the block's end;
a second block that repeats the first one's tail; input that does not compress. Purity: the same bytes in every call,
compress(A || B) = compress(A) + compress(B) on a block edge, the same stream from any round size and from the device
form. Argument errors: each gives DRM_ERR_ARG and leaves the output and the device's memory as they were. (The same
errors are also checked where there is no device at all, tests/test_bam_cpu.py.)"""
import numpy as np
import pytest

import bam_ref as B

pytestmark = pytest.mark.gpu

BLOCK = B.BLOCK


def _low(rng, n):
    """n random bytes below 128: a literal costs exactly 8 bits, so fixed Huffman never loses to stored."""
    return rng.integers(0, 128, size=n, dtype=np.uint8).tobytes()


def _checked(data):
    """(stream, BTYPE per member) of `data`, after the reader has taken the stream apart."""
    from deepreadmapper_amd import bgzf_bound, bgzf_compress
    out = bgzf_compress(data)
    raw, btypes, sizes = B.read_bgzf(out, eof=False)
    assert raw == bytes(data)
    assert sizes == [min(BLOCK, len(data) - i) for i in range(0, len(data), BLOCK)]  # byte i is in block i / 65280
    assert len(out) <= bgzf_bound(len(data))
    return out, btypes


@pytest.mark.parametrize("n", [0, 1, 3, 4, 5, 1023, 1024, 1025, BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK])
def test_block_sizes(n):
    data = _low(np.random.default_rng(n), n)
    out, btypes = _checked(data)
    assert len(btypes) == -(-n // BLOCK)
    if n == 0:
        assert out == b""
    if n == BLOCK + 1:
        assert len(B.read_bgzf(out, eof=False)[2]) == 2 and B.read_bgzf(out, eof=False)[2][1] == 1


def test_a_run_of_zeros_is_a_few_hundred_bytes():
    out, btypes = _checked(bytes(BLOCK))
    # 253 matches of 258 at no more than 26 bits each come to 823 bytes, plus the member's 26
    assert btypes == [1] and len(out) < 1000, len(out)


def test_a_repeated_record_compresses_to_less_than_a_quarter():
    data = _low(np.random.default_rng(11), 300) * 200
    out, btypes = _checked(data)
    assert btypes == [1] and 4 * len(out) < len(data), (len(out), len(data))


def test_every_match_length():
    """300 random bytes, a motif of L bytes, the motif again, one byte that differs from the motif's first: the second
    motif can only be a match of exactly L. Found, it saves L bytes less a token of at most four; not found, nothing."""
    rng = np.random.default_rng(258)
    total_in = total_out = 0
    for L in range(3, 259):
        motif = _low(rng, L)
        data = _low(rng, 300) + motif + motif + bytes([(motif[0] + 1) % 128])
        out, btypes = _checked(data)
        assert btypes == [1], L
        total_in += len(data)
        total_out += len(out)
    sum_l = sum(range(3, 259))
    print(f"every match length: {total_in} bytes in, {total_out} out, bound {total_in - sum_l // 2}")
    assert total_out <= total_in - sum_l // 2, (total_in, total_out, sum_l)


@pytest.mark.parametrize("d", [-1, 0, 1])
def test_the_distance_limit(d):
    """A 64-byte motif at offset 0 and again at 32,768 + d: a distance of 32,769 would not inflate."""
    rng = np.random.default_rng(40 + d)
    motif = _low(rng, 64)
    data = motif + _low(rng, 32768 + d - 64) + motif + _low(rng, 500)
    assert data[32768 + d:32768 + d + 64] == motif
    out, btypes = _checked(data)
    assert btypes == [1]


@pytest.mark.parametrize("j", [0, 1, 2, 3])
def test_a_match_is_cut_at_the_blocks_last_byte(j):
    """A block of 65,280 - j bytes that ends 25 bytes into the repeat of a 40-byte motif: the last match must stop at the
    block's last byte. With j = 0 the input then goes on with the rest of the motif, in a second block that cannot
    reach back for it."""
    rng = np.random.default_rng(50 + j)
    motif = _low(rng, 40)
    n = BLOCK - j
    data = _low(rng, n - 25 - 2000) + motif + _low(rng, 2000 - 40) + motif[:25]
    assert len(data) == n
    out, btypes = _checked(data)
    assert btypes == [1] and len(out) <= n + 28 - 15  # the 25 bytes as one match save at least 20 of them
    if j == 0:
        more, btypes = _checked(data + motif[25:] + _low(rng, 300))
        assert btypes == [1, 1] and more[:len(out)] == out


def test_the_last_ten_bytes_repeat_an_earlier_motif():
    rng = np.random.default_rng(60)
    motif = _low(rng, 10)
    for n in (700, 1024, 1030, 5000):
        data = _low(rng, 100) + motif + _low(rng, n - 120) + motif
        out, btypes = _checked(data)
        assert btypes == [1] and len(out) <= len(data) + 26 + 2 - 5, n  # the ten bytes as one match: at least 5 saved


def test_the_second_block_repeats_the_first_ones_tail():
    rng = np.random.default_rng(70)
    first = _low(rng, BLOCK)
    data = first + first[-1000:] + _low(rng, 3000)
    out, btypes = _checked(data)  # the reader inflates each member alone
    assert btypes == [1, 1]
    from deepreadmapper_amd import bgzf_compress
    assert out[len(bgzf_compress(first)):] == bgzf_compress(data[BLOCK:])


def test_incompressible_input_is_stored():
    rng = np.random.default_rng(80)
    out, btypes = _checked(rng.integers(0, 256, size=BLOCK, dtype=np.uint8).tobytes())
    assert btypes == [0] and len(out) == BLOCK + 31
    out, btypes = _checked(rng.integers(144, 256, size=100, dtype=np.uint8).tobytes())
    assert btypes == [0] and len(out) == 100 + 31
    out, btypes = _checked(bytes(rng.permutation(144)[:100].astype(np.uint8)))
    assert btypes == [1] and len(out) == 18 + 102 + 8  # 3 + 800 + 7 bits


def test_the_stream_is_a_function_of_the_bytes(monkeypatch):
    from deepreadmapper_amd import DrmError, bgzf_compress
    rng = np.random.default_rng(90)
    a = (_low(rng, 300) * 500)[:2 * BLOCK]
    b = _low(rng, 777) * 9
    assert len(a) == 2 * BLOCK
    ab = bgzf_compress(a + b)
    assert ab == bgzf_compress(a + b)
    assert ab == bgzf_compress(a) + bgzf_compress(b)
    # the same block wherever it sits in a call
    assert bgzf_compress(b + bytes(BLOCK - len(b)) + a)[-len(bgzf_compress(a)):] == bgzf_compress(a)
    # the rounds of the host form: DRM_BGZF_ROUND is read at every call
    for blocks in ("1", "2"):
        monkeypatch.setenv("DRM_BGZF_ROUND", blocks)
        assert bgzf_compress(a + b) == ab, blocks
    for bad in ("0", "x", "", "3 "):
        monkeypatch.setenv("DRM_BGZF_ROUND", bad)
        with pytest.raises(DrmError):
            bgzf_compress(a)
    monkeypatch.delenv("DRM_BGZF_ROUND")
    B.read_bgzf(ab, eof=False)


def test_the_device_form_gives_the_same_stream_and_the_members_sizes():
    from deepreadmapper_amd import bgzf_compress, bgzf_compress_device
    from deepreadmapper_amd.device import DeviceBuffer, synchronize
    rng = np.random.default_rng(100)
    data = _low(rng, 300) * 250 + rng.integers(0, 256, size=BLOCK, dtype=np.uint8).tobytes() + _low(rng, 5)
    want = bgzf_compress(data)
    for shift in (0, 1):  # the input at an odd device address as well
        d_data = DeviceBuffer.from_host(np.frombuffer(bytes(shift) + data, dtype=np.uint8))
        d_out, d_sizes = bgzf_compress_device(d_data.ptr + shift, len(data))
        synchronize()
        sizes = d_sizes.download()
        assert len(sizes) == -(-len(data) // BLOCK) and int(sizes.sum()) == len(want)
        assert d_out.download()[:len(want)].tobytes() == want
        at = 0
        for s in sizes:  # every size is its member's BSIZE
            assert int.from_bytes(want[at + 16:at + 18], "little") + 1 == s
            at += int(s)
        for b in (d_data, d_out, d_sizes):
            b.free()


def test_argument_errors_launch_nothing():
    """Every listed error returns DRM_ERR_ARG with the output untouched: the host form's buffer and byte count, and for
    the device form the device buffers, which hold their fill after a synchronisation."""
    import ctypes as C
    from deepreadmapper_amd import bgzf_bound, bgzf_compress, bgzf_workspace
    from deepreadmapper_amd._native import DRM_ERR_ARG, lib
    from deepreadmapper_amd.device import DeviceBuffer, synchronize
    L = lib()
    data = np.arange(100, dtype=np.uint8)
    out = np.full(bgzf_bound(100), 0xAB, dtype=np.uint8)
    got = C.c_size_t(77)
    d, o = data.ctypes.data, out.ctypes.data
    for args in ((None, 100, 0, o, out.nbytes), (d, 100, 0, None, out.nbytes), (d, -1, 0, o, out.nbytes),
                 (d, 100, 0, o, bgzf_bound(100) - 1), (d, 100, -1, o, out.nbytes)):
        assert L.drm_bgzf_compress(*args, C.byref(got)) == DRM_ERR_ARG, args
        assert (out == 0xAB).all() and got.value in (0, 77)
    assert L.drm_bgzf_compress(d, 100, 0, o, out.nbytes, None) == DRM_ERR_ARG and (out == 0xAB).all()
    assert L.drm_bgzf_compress(None, 0, 0, None, 0, C.byref(got)) == 0 and got.value == 0
    d_data = DeviceBuffer.from_host(data)
    d_out = DeviceBuffer.from_host(out)
    d_sizes = DeviceBuffer.from_host(np.full(1, 0xABABABAB, dtype=np.uint32))
    need = bgzf_workspace(100)
    work = DeviceBuffer.from_host(np.full(need, 0xAB, dtype=np.uint8))
    for args in ((None, 100, d_out.ptr, d_sizes.ptr, work.ptr, need), (d_data.ptr, 100, None, d_sizes.ptr, work.ptr, need),
                 (d_data.ptr, 100, d_out.ptr, None, work.ptr, need), (d_data.ptr, 100, d_out.ptr, d_sizes.ptr, None, need),
                 (d_data.ptr, 100, d_out.ptr, d_sizes.ptr, work.ptr, need - 1),
                 (d_data.ptr, -100, d_out.ptr, d_sizes.ptr, work.ptr, need)):
        assert L.drm_bgzf_compress_device(*args, None) == DRM_ERR_ARG, args
    synchronize()
    assert (d_out.download() == 0xAB).all() and d_sizes.download()[0] == 0xABABABAB and (work.download() == 0xAB).all()
    assert L.drm_bgzf_compress_device(None, 0, None, None, None, 0, None) == 0
    for b in (d_data, d_out, d_sizes, work):
        b.free()
    assert B.read_bgzf(bgzf_compress(data.tobytes()), eof=False)[0] == data.tobytes()  # and the good call still works
