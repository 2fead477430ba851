"""The zstd decode on the GPU (tsg_inflate_zstd_device; zstdec.hip): on every
group of tests/_zstd_corpus.py the device call equals the CPU model
(tsg_test_zstd_model) in output bytes, out_lens, status, return code and
message, writes nothing outside the streams' outputs and leaves d_z alone; the
whole corpus in one launch and again in reverse order; exact and short slots;
InflateZstdDevice's slots from the size bound and its regrowth from small caps;
one stream of 64 frames (4 MiB of output); streams of 300 frames, whose
records need a second launch, beside ordinary ones; and the chain
ScanLayersCompressedDevice on gzip, zstd and plain layers against
PrepareLayerTar(scan=True) on the plain tars and the oracle's analyzer."""
import ctypes
import gzip

import numpy as np
import pytest

import _zstd_corpus as Z
from oracle import secret_oracle as so
from oracle import walker_oracle as wo
from trivy_amd import _lib
from trivy_amd import secret as S

pytestmark = pytest.mark.gpu
CORPUS = Z.corpus()
_sc = []


def scanner():
    if not _sc:
        _sc.append(S.Scanner(None))
    return _sc[0]


def run_device(streams, caps):
    """tsg_inflate_zstd_device like Z.run_model: (rc, message, status, out_lens, dst without the guards, dst_offsets)"""
    import torch
    L = _lib.lib()
    buf, zo, do = Z.pack(streams, caps)
    n = len(zo) - 1
    d_z = torch.from_numpy(buf).to("cuda:0")
    dst = torch.full((int(do[-1]) + 2 * Z.GUARD,), Z.FILL, dtype=torch.uint8, device="cuda:0")
    out_lens, status = np.zeros(n, np.uint64), np.full(n, -1, np.int32)
    torch.cuda.synchronize()
    ms = ctypes.c_double()
    rc = L.tsg_inflate_zstd_device(scanner().engine(), ctypes.c_void_p(d_z.data_ptr()), zo.ctypes.data, n,
                                   ctypes.c_void_p(dst.data_ptr() + Z.GUARD), do.ctypes.data, out_lens.ctypes.data,
                                   status.ctypes.data, ctypes.byref(ms))
    msg = L.tsg_last_error().decode() if rc else ""
    h = dst.cpu().numpy()
    assert (h[:Z.GUARD] == Z.FILL).all() and (h[len(h) - Z.GUARD:] == Z.FILL).all()       # nothing outside the slots
    assert np.array_equal(d_z.cpu().numpy(), buf)                                          # d_z is unchanged
    return rc, msg, status.tolist(), out_lens.tolist(), h[Z.GUARD:len(h) - Z.GUARD], do.tolist()


def check_equals_model(cases, caps=None):
    streams = [c.z for c in cases]
    caps = [Z.default_cap(c) for c in cases] if caps is None else caps
    want = Z.run_model(streams, caps)
    got = run_device(streams, caps)
    assert got[:4] == want[:4]                   # rc, message, status, out_lens
    do, out_lens = got[5], got[3]
    for i in range(len(do) - 1):
        b = do[i]
        assert got[4][b:b + out_lens[i]].tobytes() == want[4][b:b + out_lens[i]].tobytes(), cases[i].name
    Z.check_slots(out_lens, got[4], do)
    return got


GROUPS = ["levels", "windows", "literals", "sequences", "frames", "small", "invalid"]


@pytest.mark.parametrize("group", GROUPS)
def test_device_equals_model_gpu(group):
    cases = [c for c in CORPUS.values() if c.group == group]
    assert cases
    rc, msg, status, out_lens, dst, do = check_equals_model(cases)
    assert status == [c.status for c in cases]
    for i, c in enumerate(cases):
        if c.status == Z.OK:
            assert dst[do[i]:do[i] + out_lens[i]].tobytes() == c.payload, c.name


def test_whole_corpus_in_one_launch_and_reversed_gpu():
    cases = list(CORPUS.values())
    fwd = check_equals_model(cases)
    assert fwd[2] == [c.status for c in cases]
    rev = check_equals_model(cases[::-1])
    assert rev[2] == fwd[2][::-1] and rev[3] == fwd[3][::-1]
    for i, c in enumerate(cases):
        if c.status == Z.OK:
            j = len(cases) - 1 - i
            assert rev[4][rev[5][j]:rev[5][j] + rev[3][j]].tobytes() == c.payload, c.name


@pytest.mark.parametrize("name", ["lv_text_19_c1_s1", "lv_zeros_3_c1_s0", "w10_text", "w17_far", "rle_blocks", "tiny_300",
                                  "lit_raw_fmt3", "seq_rle_long"])
def test_slot_exact_and_short_gpu(name):
    c = CORPUS[name]
    n = len(c.payload)
    rc, msg, status, out_lens, dst, do = check_equals_model([c], caps=[n])
    assert (rc, status, out_lens) == (0, [Z.OK], [n]) and dst.tobytes() == c.payload
    for cap in (n - 1, n // 2, 0):
        rc, msg, status, out_lens, dst, do = check_equals_model([c], caps=[cap])
        assert rc != 0 and status == [Z.DST_FULL] and msg == "zstd stream 0: the output does not fit its slot"
        assert (dst[out_lens[0]:] == Z.FILL).all()


def test_slots_from_the_bound_and_regrowth_from_small_caps_gpu():
    import torch
    sc = scanner()
    names = ["lv_text_3_c1_s1", "lv_text_3_c0_s0", "empty_frame", "lv_zeros_9_c1_s0", "wrong_checksum", "rle_128k", "block_type_3",
             "tiny_300", "w17_far"]
    cases = [CORPUS[n] for n in names]
    buf, zo, _ = Z.pack([c.z for c in cases], [0] * len(cases))
    d_z = torch.from_numpy(buf).to("cuda:0")

    def check(dst, do, out_lens, status):
        assert status.tolist() == [c.status for c in cases]
        h = dst.cpu().numpy()
        for i, c in enumerate(cases):
            if c.status == Z.OK:
                assert h[int(do[i]):int(do[i]) + int(out_lens[i])].tobytes() == c.payload, c.name
    # the default slots: tsg_zstd_size_bound + 64 holds every stream at the first go
    dst, do, out_lens, status, st = sc.InflateZstdDevice(d_z, zo, with_stats=True)
    check(dst, do, out_lens, status)
    assert st["rounds"] == 0
    bounds = [S.Scanner.ZstdSizeBound(c.z)[0] for c in cases]
    dst, do, out_lens, status, st = sc.InflateZstdDevice(d_z, zo, bounds=bounds, with_stats=True)
    check(dst, do, out_lens, status)
    assert st["rounds"] == 0 and [int(do[i + 1] - do[i]) for i in range(len(cases))] == [(b + 64 + 15) & ~15 for b in bounds]
    # a caller's small caps: 1 KiB doubled until 'w17_far' fits
    dst, do, out_lens, status, st = sc.InflateZstdDevice(d_z, zo, caps=[1024] * len(cases), with_stats=True)
    check(dst, do, out_lens, status)
    assert st["rounds"] == int(np.ceil(np.log2(len(CORPUS["w17_far"].payload) / 1024)))
    # a bound on the rounds leaves the stream TSG_ZSTD_DST_FULL
    _, _, _, status = sc.InflateZstdDevice(d_z, zo, caps=[1024] * len(cases), max_regrow=2)
    assert status[names.index("rle_128k")] == Z.DST_FULL and status[names.index("empty_frame")] == Z.OK


def test_stream_of_64_frames_gpu():
    names = ["seq_text", "w17_far", "zeros_long", "rle_128k", "lit_bits11", "lv_text_19_c1_s1", "seq_rle_long", "lit_huf4_fse"]
    cases = [CORPUS[n] for n in names] * 8
    z = b"".join(c.z for c in cases)
    want = b"".join(c.payload for c in cases)
    assert len(cases) == 64 and 4 << 20 <= len(want) < 8 << 20
    rc, msg, status, out_lens, dst, do = run_device([z], [len(want)])
    assert (rc, status, out_lens) == (0, [Z.OK], [len(want)]), msg
    assert dst.tobytes() == want
    frames, blocks = ctypes.c_uint64(), ctypes.c_uint64()
    _lib.lib().tsg_test_zstd_last_stats(None, None, ctypes.byref(frames), ctypes.byref(blocks))
    assert frames.value == 64 and blocks.value >= 64


def test_streams_of_many_frames_get_their_records_gpu():
    # more frames than the first launch keeps records for: those streams run again, beside streams that do not
    names = ["tiny_300", "lv_text_3_c1_s1", "skip_between", "tiny_300", "wrong_checksum"]
    cases = [CORPUS[n] for n in names]
    tiny = [f for f, _ in Z.tiny_frames()]
    tiny[298] = tiny[298][:-1] + bytes([tiny[298][-1] ^ 1])     # a wrong checksum far behind the first launch's records
    cases.append(Z.Case("tiny_300_bad_sum", "many", b"".join(tiny), None, Z.CHECKSUM))
    rc, msg, status, out_lens, dst, do = check_equals_model(cases)
    assert status == [c.status for c in cases]
    frames = ctypes.c_uint64()
    _lib.lib().tsg_test_zstd_last_stats(None, None, ctypes.byref(frames), None)
    assert frames.value == 300 * 3 + 1 + 2 + 1
    for i, c in enumerate(cases[:4]):
        assert dst[do[i]:do[i] + out_lens[i]].tobytes() == c.payload, c.name


def test_rejects_bad_arguments_gpu():
    import torch
    L = _lib.lib()
    e = scanner().engine()
    c = CORPUS["lv_text_3_c1_s1"]
    buf, zo, do = Z.pack([c.z], [len(c.payload)])
    do = np.array(do, np.uint64)
    d_z = torch.from_numpy(buf).to("cuda:0")
    dst = torch.empty(int(do[-1]) + 64, dtype=torch.uint8, device="cuda:0")
    out_lens, status = np.zeros(1, np.uint64), np.zeros(1, np.int32)
    torch.cuda.synchronize()

    def call(src, out, d=do):
        rc = L.tsg_inflate_zstd_device(e, ctypes.c_void_p(src), zo.ctypes.data, 1, ctypes.c_void_p(out), d.ctypes.data,
                                       out_lens.ctypes.data, status.ctypes.data, None)
        return rc, L.tsg_last_error().decode() if rc else ""
    assert call(buf.ctypes.data, dst.data_ptr())[1] == "zstd: buffers must be device memory of one device"
    assert call(d_z.data_ptr() + 1, dst.data_ptr())[1] == "zstd: buffers must be 16-byte aligned"
    assert call(d_z.data_ptr(), d_z.data_ptr())[1] == "zstd: d_z and d_dst must not overlap"
    assert call(d_z.data_ptr(), dst.data_ptr(), do + np.uint64(8))[1] == "zstd: every slot must start 16-byte aligned"
    assert call(d_z.data_ptr(), dst.data_ptr()) == (0, "")
    assert dst[:len(c.payload)].cpu().numpy().tobytes() == c.payload


def test_chain_on_mixed_layers_equals_host_route_and_oracle_gpu():
    sc = scanner()
    tars = Z.layer_tars()
    order = ["content", "pax", "smoke", "names", "pax"]
    blobs = [Z.load("layer_content"), gzip.compress(tars["pax"], 6, mtime=0), Z.load("layer_smoke"), tars["names"], tars["pax"]]
    assert [S.Scanner.LayerCompression(b) for b in blobs] == [_lib.LAYER_ZSTD, _lib.LAYER_GZIP, _lib.LAYER_ZSTD, _lib.LAYER_NONE,
                                                             _lib.LAYER_NONE]
    layers, st = sc.ScanLayersCompressedDevice(blobs, with_stats=True, contents=True)
    assert st["zstd_bytes"] == len(blobs[0]) + len(blobs[2]) and st["gz_bytes"] == len(blobs[1])
    assert st["plain_bytes"] == len(blobs[3]) + len(blobs[4]) and st["tar_bytes"] == sum(len(tars[k]) for k in order)
    nfind = 0
    for key, (args, walk, secrets) in zip(order, layers):
        tar = tars[key]
        hargs, hwalk, hsecrets = S.PrepareLayerTar(sc, tar, scan=True)
        assert walk == hwalk
        assert args == hargs
        assert secrets == hsecrets
        files, _, _ = wo.walk(tar, (), ())       # the oracle's walk and Analyze per file
        by_file = {a.FilePath: s for a, s in zip(args, secrets)}
        a = so.SecretAnalyzer("")
        for p, raw in files:
            want = a.analyze(p, raw, dir_="") if a.required(p, len(raw)) else None
            if want is None:
                assert not (by_file.get("/" + p) or {}).get("Findings"), p
            else:
                assert by_file["/" + p] == want[0], p
                nfind += len(want[0]["Findings"])
    assert nfind >= 3
    # without contents=True the prepared bytes stay on the device
    one = sc.ScanLayersCompressedDevice([blobs[2]])[0]
    assert one[1:] == layers[2][1:] and all(a.Content is None for a in one[0])
    # a failed stream names its blob and the status: a wrong checksum, a corrupt block, a cut, a gzip layer's own text
    bad = bytearray(blobs[2])
    bad[-1] ^= 0x55
    with pytest.raises(S.WalkError, match="^layer 2: zstd: invalid checksum$"):
        sc.ScanLayersCompressedDevice([blobs[0], blobs[1], bytes(bad)])
    with pytest.raises(S.WalkError, match="^layer 1: zstd: corrupt input$"):
        sc.ScanLayersCompressedDevice([blobs[3], CORPUS["block_type_3"].z, blobs[0]])
    with pytest.raises(S.WalkError, match="^layer 0: zstd: unexpected end of input$"):
        sc.ScanLayersCompressedDevice([blobs[0][:-3], blobs[1]])
    with pytest.raises(S.WalkError, match="^layer 1: unexpected EOF$"):
        sc.ScanLayersCompressedDevice([blobs[0], blobs[1][:-3]])
