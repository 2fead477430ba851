"""Host-side mirror of github.com/aquasecurity/trivy/pkg/fanal/secret.

Same names, argument meaning and error behaviour as the reference package
(pkg/fanal/secret/scanner.go), backed by the MI355X engine behind the C-ABI in
include/trivy_secret.h:

  ParseConfig(config_path) -> Config | None     scanner.go:277-307
  NewScanner(config)       -> Scanner           scanner.go:320-364
  Scanner.Scan(ScanArgs)   -> types.Secret      scanner.go:377-463
  Scanner.ScanBatch([ScanArgs]) -> [types.Secret]   (batched entry)
  GetBuiltinRules()                             builtin-rules.go:87-89
  GetSecretRulesMetadata()                      builtin-rules.go:91-99

types.Secret is returned as a dict with the Go field names
({"FilePath", "Findings": [{"RuleID", ..., "Code": {"Lines": [...]}, "Match"}]});
Go byte strings are decoded with 'surrogateescape'.  Scan runs on the GPU; a
machine without a HIP device raises instead of silently scanning on the CPU.
"""
import collections.abc
import ctypes
import json
import os
from dataclasses import dataclass

import numpy as np
import yaml

from . import _lib


class ConfigError(Exception):
    """ParseConfig failure (file open, YAML decode, regexp compile)."""


class _GoStringLoader(yaml.SafeLoader):
    """yaml.SafeLoader that keeps every plain scalar a string (yaml.v3 decoding
    into the string fields of secret.Config), except null."""


_GoStringLoader.yaml_implicit_resolvers = {
    k: [(tag, rx) for tag, rx in v if tag == "tag:yaml.org,2002:null"]
    for k, v in yaml.SafeLoader.yaml_implicit_resolvers.items()
}


def load_yaml(path):
    """yaml.v3 Decoder.Decode of the file's FIRST document.  An input with no
    document at all (empty, or only comments) is io.EOF, which ParseConfig
    reports as "secrets config decode error: EOF" (scanner.go:296-298); an
    explicit null document decodes to the zero Config."""
    with open(path, "rb") as f:
        text = f.read()
    docs = yaml.load_all(text, Loader=_GoStringLoader)  # noqa: S506 (SafeLoader subclass)
    try:
        return next(docs)
    except StopIteration:
        raise ConfigError("secrets config decode error: EOF") from None


@dataclass
class ScanArgs:                       # scanner.go:366-370
    FilePath: str
    Content: bytes
    Binary: bool = False


def ParseConfig(config_path):
    """nil for an empty path or a missing file (builtin rules only)."""
    if not config_path:
        return None
    if not os.path.exists(config_path):
        return None
    try:
        doc = load_yaml(config_path)
    except yaml.YAMLError as e:
        raise ConfigError("secrets config decode error: %s" % e)
    if doc is None:                    # explicit null document: zero Config
        doc = {}
    if not isinstance(doc, dict):
        raise ConfigError("secrets config decode error: not a mapping")
    return doc


def GetBuiltinRules():
    return json.loads(_lib.lib().tsg_builtin_rules_json().decode("utf-8"))["rules"]


def GetSecretRulesMetadata():
    """builtin-rules.go:91-99: [{"name": rule ID, "description": rule title}]
    (iacRules.Check's json form) for the builtin rules."""
    return json.loads(_lib.lib().tsg_secret_rules_metadata_json().decode("utf-8"))


def _device_default():
    v = os.environ.get("TSG_DEVICE") or os.environ.get("LOCAL_RANK") or "0"
    return int(v)


class Scanner:
    """NewScanner(config) + Scan.  The ruleset is compiled once; the GPU
    engine is created on first use on `device` (default LOCAL_RANK or 0)."""

    def __init__(self, config=None, device=None, threads=0):
        L = _lib.lib()
        rs = ctypes.c_void_p()
        if config is None:
            _lib.check(L.tsg_ruleset_compile(None, 0, ctypes.byref(rs)))
        else:
            js = json.dumps(config, ensure_ascii=True).encode("utf-8")
            rc = L.tsg_ruleset_compile(js, len(js), ctypes.byref(rs))
            if rc != 0:
                raise ConfigError(L.tsg_last_error().decode("utf-8", "replace"))
        self._rs = rs
        self._engine = None
        self._device = _device_default() if device is None else device
        self._threads = threads

    def __del__(self):
        try:
            L = _lib.lib()
            if self._engine:
                L.tsg_engine_destroy(self._engine)
            if self._rs:
                L.tsg_ruleset_free(self._rs)
        except Exception:
            pass

    @property
    def rule_ids(self):
        L = _lib.lib()
        return [L.tsg_ruleset_rule_id(self._rs, i).decode("utf-8", "surrogateescape")
                for i in range(L.tsg_ruleset_num_rules(self._rs))]

    def AllowPath(self, path):          # scanner.go:56-59
        b = path.encode("utf-8", "surrogateescape")
        return _lib.lib().tsg_ruleset_allow_path(self._rs, b, len(b)) == 1

    def engine(self):
        if self._engine is None:
            L = _lib.lib()
            e = ctypes.c_void_p()
            mask = 0 if self._device == "all" else (1 << int(self._device))
            _lib.check(L.tsg_engine_create(self._rs, mask, ctypes.byref(e)))
            if self._threads:
                L.tsg_engine_set_threads(e, self._threads)
            self._engine = e
        return self._engine

    def report(self):
        return _lib.lib().tsg_engine_report(self.engine()).decode("utf-8", "replace")

    def StripCR(self, d_src, d_offsets, nfiles, total):
        """GPU-side CR strip (tsg_strip_cr_device) of a device-resident batch of
        text files: every file's bytes.ReplaceAll(content, "\r", "")
        (pkg/fanal/analyzer/secret/secret.go:121) in one pass.

        d_src: uint8 device tensor holding >= total bytes (16-byte aligned);
        d_offsets: int64 device tensor of nfiles + 1 file starts (0 ... total).
        Returns (d_dst, d_new_offsets, stripped_total, kernel_ms); d_dst holds
        stripped_total bytes (plus 64 bytes of padding for the resident scan).
        """
        import torch
        dev = d_src.device
        dst = torch.empty(int(total) + 64, dtype=torch.uint8, device=dev)
        new_off = torch.empty(int(nfiles) + 1, dtype=torch.int64, device=dev)
        torch.cuda.current_stream(dev).synchronize()     # the engine runs on its own stream
        out_total, ms = ctypes.c_uint64(), ctypes.c_double()
        _lib.check(_lib.lib().tsg_strip_cr_device(self.engine(), ctypes.c_void_p(d_src.data_ptr()),
                                                   ctypes.c_void_p(d_offsets.data_ptr()), int(nfiles), int(total),
                                                   ctypes.c_void_p(dst.data_ptr()),
                                                   ctypes.c_void_p(new_off.data_ptr()), ctypes.byref(out_total),
                                                   ctypes.byref(ms)))
        return dst, new_off, out_total.value, ms.value

    def PrepareBatchDevice(self, d_raw, raw_offsets, paths, config_path="", file_patterns=(), image=False,
                           threads=0, dst_cap=None, with_passes=False):
        """The analyzer's whole content preparation on the GPU
        (tsg_prepare_batch_device; pkg/fanal/analyzer/secret/secret.go:103-150)
        for a raw batch that lives in HBM: the device twin of PrepareBatch.

        d_raw: uint8 device tensor, the files as read, back to back (16-byte
        aligned); raw_offsets: nfiles + 1 host integers (0 ... total); paths:
        input.FilePath of every file.  The gate (file_patterns, Required with
        config_path) runs on the host from the paths and sizes; the device
        classifies every file by its first 300 bytes (utils.IsBinary), drops
        binaries other than .pyc, strips CR from text and extracts the
        printable runs of binary .pyc files (utils.ExtractPrintableBytes),
        packing the kept contents into a new tensor of total + (number of .pyc
        paths) + 64 bytes (dst_cap: another size, for tests).

        Returns (d_dst, offsets, scan_paths, index, binary, kernel_ms) for the
        kept files: offsets (nkept + 1, uint64) cut d_dst, index[k] is kept
        file k's place in `paths`, scan_paths its ScanArgs.FilePath (image=True
        adds the "/" prefix, secret.go:133-135), binary its ScanArgs.Binary.
        with_passes appends the kernel times of classify, count, scan, compact.
        The scan to follow is ScanBatchDevice(d_dst, offsets, scan_paths, binary)."""
        import torch
        L = _lib.lib()
        off = np.ascontiguousarray(raw_offsets, dtype=np.uint64)
        nfiles = len(off) - 1
        if nfiles != len(paths):
            raise ValueError("raw_offsets must hold one more entry than paths")
        total = int(off[-1]) if nfiles else 0
        if d_raw.dtype != torch.uint8 or not d_raw.is_cuda or not d_raw.is_contiguous():
            raise ValueError("d_raw must be a contiguous uint8 device tensor")
        if d_raw.numel() < total:
            raise ValueError("d_raw is shorter than the batch")
        enc = [p.encode("utf-8", "surrogateescape") if isinstance(p, str) else bytes(p) for p in paths]
        if dst_cap is None:
            dst_cap = total + sum(1 for p in enc if p.endswith(b".pyc")) + 64
        dst = torch.empty(max(int(dst_cap), 16), dtype=torch.uint8, device=d_raw.device)
        cpaths, lens, _keep = _lib.pack_paths(enc)
        o, keep = _lib.feed_opts(config_path, file_patterns, threads=threads)
        torch.cuda.current_stream(d_raw.device).synchronize()     # the engine runs on its own stream
        h, ms = ctypes.c_void_p(), ctypes.c_double()
        rc = L.tsg_prepare_batch_device(self.engine(), ctypes.c_void_p(d_raw.data_ptr()), off.ctypes.data, nfiles,
                                        cpaths, lens, ctypes.byref(o), ctypes.c_void_p(dst.data_ptr()), int(dst_cap),
                                        ctypes.byref(h), ctypes.byref(ms))
        del keep
        _lib.check(rc)
        try:
            offs, idx, binf, _data = _prepared_view(L, h)
            passes = (ctypes.c_double * 4)()
            _lib.check(L.tsg_prepared_pass_ms(h, passes))
        finally:
            L.tsg_prepared_free(h)
        scan_paths = [("/" if image else "") + paths[i] for i in idx]
        out = (dst, offs, scan_paths, idx, binf, ms.value)
        return out + (list(passes),) if with_passes else out

    def PrepareLayerTarDevice(self, d_tar, length=None, skip_files=(), skip_dirs=(), file_patterns=(), config_path="",
                              threads=0, dst_cap=None, with_stats=False):
        """One container layer whose uncompressed tar lives in HBM
        (tsg_prepare_layer_tar_device): walker.LayerTar.Walk
        (pkg/fanal/walker/tar.go:35-103) and the analyzer's content preparation
        without the tar crossing the link -- the device twin of PrepareLayerTar.

        d_tar: uint8 device tensor (16-byte aligned), of which the first
        `length` bytes (default: all) are the tar.  The GPU marks the blocks
        the walk may read (headers by their checksum, PAX / GNU long-name
        payloads) and stores them into host-mapped memory; the walk runs on the
        host over them; the content pass then packs the kept files' prepared
        contents into a new tensor of length + 64 bytes (dst_cap: another size,
        for tests).

        Returns (d_dst, offsets, scan_paths, binary, walk, kernel_ms): offsets
        (nkept + 1, uint64) cut d_dst, scan_paths are the "/"-prefixed image
        paths, walk the dict PrepareLayerTar returns.  with_stats appends a
        dict of the device walk (blocks, marked, gathered_bytes,
        fallback_reads, retries, scan_ms, pass_ms).  Raises WalkError on a
        malformed tar.  The scan to follow is
        ScanBatchDevice(d_dst, offsets, scan_paths, binary)."""
        import torch
        L = _lib.lib()
        if d_tar.dtype != torch.uint8 or not d_tar.is_cuda or not d_tar.is_contiguous():
            raise ValueError("d_tar must be a contiguous uint8 device tensor")
        n = d_tar.numel() if length is None else int(length)
        if n < 0 or n > d_tar.numel():
            raise ValueError("length is past the end of d_tar")
        if d_tar.data_ptr() & 15:
            raise ValueError("d_tar must be 16-byte aligned")
        if dst_cap is None:
            dst_cap = n + 64
        dst = torch.empty(max(int(dst_cap), 16), dtype=torch.uint8, device=d_tar.device)
        o, keep = _lib.feed_opts(config_path, file_patterns, skip_files, skip_dirs, threads=threads)
        torch.cuda.current_stream(d_tar.device).synchronize()     # the engine runs on its own stream
        h, ms = ctypes.c_void_p(), ctypes.c_double()
        rc = L.tsg_prepare_layer_tar_device(self.engine(), ctypes.c_void_p(d_tar.data_ptr()), n, ctypes.byref(o),
                                            ctypes.c_void_p(dst.data_ptr()), int(dst_cap), ctypes.byref(h),
                                            ctypes.byref(ms))
        del keep
        if rc != 0:
            msg = L.tsg_last_error().decode("utf-8", "replace")
            if msg.startswith("failed to extract the archive:"):
                raise WalkError(msg)
            _lib.check(rc)
        try:
            offs, _idx, binf, _data = _prepared_view(L, h)
            walk = json.loads(L.tsg_prepared_walk_json(h).decode("utf-8", "surrogateescape"))
            pp, pl = ctypes.POINTER(ctypes.c_char_p)(), ctypes.POINTER(ctypes.c_uint32)()
            _lib.check(L.tsg_prepared_paths(h, ctypes.byref(pp), ctypes.byref(pl)))
            scan_paths = [ctypes.string_at(pp[k], pl[k]).decode("utf-8", "surrogateescape") for k in range(len(binf))]
            out = (dst, offs, scan_paths, binf, walk, ms.value)
            if not with_stats:
                return out
            blocks, marked, gbytes = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
            fb, retries, scan_ms = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_double()
            _lib.check(L.tsg_prepared_tar_stats(h, ctypes.byref(blocks), ctypes.byref(marked), ctypes.byref(gbytes),
                                                ctypes.byref(fb), ctypes.byref(retries), ctypes.byref(scan_ms)))
            passes = (ctypes.c_double * 4)()
            _lib.check(L.tsg_prepared_pass_ms(h, passes))
            return out + ({"blocks": blocks.value, "marked": marked.value, "gathered_bytes": gbytes.value,
                           "fallback_reads": fb.value, "retries": retries.value, "scan_ms": scan_ms.value,
                           "pass_ms": list(passes)},)
        finally:
            L.tsg_prepared_free(h)

    def InflateGzipDevice(self, d_gz, gz_offsets, caps=None, hints=None, max_regrow=9, with_stats=False):
        """A batch of gzip streams that lies in HBM, inflated there
        (tsg_inflate_gzip_device): layer.Uncompressed() of
        pkg/fanal/artifact/image/image.go:464-492 -- Go's compress/gzip,
        multistream -- for all layers at once, one wavefront per stream.

        d_gz: uint8 device tensor (16-byte aligned, 16 readable bytes behind
        the last stream); gz_offsets: nstreams + 1 host integers, stream i =
        d_gz[gz_offsets[i]:gz_offsets[i + 1]].  caps: each stream's slot size;
        default max(size hint, 4 * compressed length) + 64, rounded up to 16
        bytes, where the size hint is the last member's ISIZE (hints: the
        caller's, else read from d_gz: four bytes per stream cross the link).
        A stream whose output does not fit (TSG_INFLATE_DST_FULL) is run again
        in a slot twice as large, at most max_regrow times; only those streams
        run again, the others' outputs are copied on the device.

        Returns (d_dst, dst_offsets, out_lens, status): stream i's output is
        d_dst[dst_offsets[i]:dst_offsets[i] + out_lens[i]], status[i] its
        TSG_INFLATE_* value (_lib.INFLATE_OK ...; the text:
        tsg_inflate_status_text).  A failed stream raises nothing here: its
        neighbours' outputs are valid.  with_stats appends {"ms": kernel time,
        "rounds": launches after the first}."""
        import torch
        L = _lib.lib()
        go = np.ascontiguousarray(gz_offsets, dtype=np.uint64)
        n = len(go) - 1
        if n < 0:
            raise ValueError("gz_offsets must hold at least one entry")
        if d_gz.dtype != torch.uint8 or not d_gz.is_cuda or not d_gz.is_contiguous() or d_gz.data_ptr() & 15:
            raise ValueError("d_gz must be a contiguous, 16-byte aligned uint8 device tensor")
        if n and d_gz.numel() < int(go[-1]):
            raise ValueError("d_gz is shorter than the batch")
        clen = (go[1:] - go[:-1]).astype(np.int64)
        if caps is None:
            if hints is None:
                hints = np.zeros(n, np.int64)
                big = np.flatnonzero(clen >= 18)
                if len(big):
                    at = torch.from_numpy((go[1:][big].astype(np.int64) - 4)[:, None] + np.arange(4)).to(d_gz.device)
                    tail = d_gz[at].cpu().numpy().astype(np.int64)
                    hints[big] = tail[:, 0] | tail[:, 1] << 8 | tail[:, 2] << 16 | tail[:, 3] << 24
            caps = np.maximum(np.asarray(hints, np.int64), 4 * clen) + 64
        caps = (np.asarray(caps, np.int64) + 15) & ~15 if n else np.zeros(0, np.int64)
        if len(caps) != n:
            raise ValueError("caps must hold one entry per stream")
        status = np.full(n, _lib.INFLATE_DST_FULL, np.int32)
        out_lens = np.zeros(n, np.uint64)
        dst, do, ms, rounds = None, None, 0.0, 0
        torch.cuda.current_stream(d_gz.device).synchronize()     # the call runs on its own stream
        while True:
            new_do = np.zeros(n + 1, np.uint64)
            np.cumsum(caps, out=new_do[1:])
            new = torch.empty(max(int(new_do[-1]), 16) + 16, dtype=torch.uint8, device=d_gz.device)
            todo = np.flatnonzero(status == _lib.INFLATE_DST_FULL)
            if dst is not None:                  # what is done moves over on the device
                for i in np.flatnonzero(status != _lib.INFLATE_DST_FULL):
                    k = int(out_lens[i])
                    new[int(new_do[i]):int(new_do[i]) + k] = dst[int(do[i]):int(do[i]) + k]
                torch.cuda.current_stream(d_gz.device).synchronize()
            dst, do = new, new_do
            runs = np.split(todo, np.flatnonzero(np.diff(todo) != 1) + 1) if len(todo) else []
            for run in runs:                     # adjacent streams go in one launch
                a, b = int(run[0]), int(run[-1]) + 1
                g, d = np.ascontiguousarray(go[a:b + 1]), np.ascontiguousarray(do[a:b + 1])
                t = ctypes.c_double()
                rc = L.tsg_inflate_gzip_device(self.engine(), ctypes.c_void_p(d_gz.data_ptr()), g.ctypes.data, b - a,
                                               ctypes.c_void_p(dst.data_ptr()), d.ctypes.data,
                                               out_lens[a:b].ctypes.data, status[a:b].ctypes.data, ctypes.byref(t))
                if rc != 0 and not L.tsg_last_error().startswith(b"gzip stream "):
                    _lib.check(rc)               # the call itself failed, not a stream
                ms += t.value
            full = status == _lib.INFLATE_DST_FULL
            if not full.any() or rounds >= max_regrow:
                break
            rounds += 1
            caps = np.where(full, caps * 2, caps)
        out = (dst, do, out_lens, status)
        return out + ({"ms": ms, "rounds": rounds},) if with_stats else out

    def ScanLayersGzipDevice(self, blobs, skip_files=(), skip_dirs=(), file_patterns=(), config_path="",
                             with_stats=False, contents=False, window=None, window_lines=None):
        """The layers of an image as the registry or `docker save` hands them
        over -- one gzip stream each -- scanned with only the compressed bytes
        and the confirmer's gather crossing the link:

            one upload of all blobs -> InflateGzipDevice (one launch for all
            layers) -> per layer PrepareLayerTarDevice -> ScanBatchDevice

        blobs: a list of bytes-like objects (bytes, or pinned buffers such as a
        pinned uint8 torch tensor or a numpy view of one).  Returns, per
        layer, what PrepareLayerTar(scanner, tar, ..., scan=True) returns for
        the gunzipped tar: (ScanArgs list, walk dict, [types.Secret]) -- except
        that the prepared contents stay on the device: ScanArgs.Content is
        None unless contents=True downloads them.  A layer that does not
        inflate raises WalkError with its index and Go's text
        ("unexpected EOF", "gzip: invalid checksum", ...); a malformed tar
        raises WalkError as PrepareLayerTarDevice does.  with_stats appends
        {"gz_bytes", "tar_bytes", "inflate_ms", "inflate_rounds"} to the list's
        tuple: (layers, stats).  window, window_lines: ScanBatchDevice's, for
        every layer's scan."""
        if window_lines is not None and window is None:
            raise ValueError("window_lines needs window=(before, after, min_file)")
        views = self._blob_views(blobs)
        opts = dict(skip_files=skip_files, skip_dirs=skip_dirs, file_patterns=file_patterns, config_path=config_path)
        slots, st = self._gzip_layer_slots(views, list(range(len(views))))
        layers = [self._scan_layer_slot(d_tar, k, opts, contents, window, window_lines) for d_tar, k in slots]
        if with_stats:
            return layers, {"gz_bytes": st["gz_bytes"], "tar_bytes": sum(k for _, k in slots), "inflate_ms": st["ms"],
                            "inflate_rounds": st["rounds"]}
        return layers

    # ---- what ScanLayersGzipDevice and ScanLayersCompressedDevice share ----
    @staticmethod
    def _blob_views(blobs):
        import torch
        return [b.numpy() if isinstance(b, torch.Tensor) else np.frombuffer(b, dtype=np.uint8) for b in blobs]

    def _upload_blobs(self, views, idx, align=1):
        """views[i] for i in idx, each starting at a multiple of align, through one pinned buffer in one copy:
        (device tensor with 16 zero bytes behind the last blob, offsets of len(idx) + 1)"""
        import torch
        off = np.zeros(len(idx) + 1, np.uint64)
        if idx:
            np.cumsum([(len(views[i]) + align - 1) // align * align for i in idx], out=off[1:])
        dev = torch.device("cuda", 0 if self._device == "all" else int(self._device))
        host = torch.empty(int(off[-1]) + 16, dtype=torch.uint8).pin_memory()
        hv = host.numpy()
        for k, i in enumerate(idx):
            a = int(off[k])
            hv[a:a + len(views[i])] = views[i]
            hv[a + len(views[i]):int(off[k + 1])] = 0
        hv[int(off[-1]):] = 0
        return host.to(dev, non_blocking=True), off

    def _gzip_layer_slots(self, views, idx):
        """The gzip blobs views[i], i in idx: one upload, one InflateGzipDevice.  ([(slot tensor, tar length)] in
        idx's order, {"gz_bytes", "ms", "rounds"}); a stream that fails raises WalkError with its index i."""
        L = _lib.lib()
        hints = np.zeros(len(idx), np.int64)
        for k, i in enumerate(idx):
            h = ctypes.c_uint64()
            if len(views[i]) and L.tsg_gzip_size_hint(views[i].ctypes.data, len(views[i]), ctypes.byref(h)) == 0:
                hints[k] = h.value
        d_gz, go = self._upload_blobs(views, idx)   # the one upload
        dst, do, out_lens, status, ist = self.InflateGzipDevice(d_gz, go, hints=hints, with_stats=True)
        for k, i in enumerate(idx):
            if status[k] != _lib.INFLATE_OK:
                text = L.tsg_inflate_status_text(int(status[k])).decode() or "the inflated layer does not fit its slot"
                raise WalkError("layer %d: %s" % (i, text))
        slots = [(dst[int(do[k]):int(do[k + 1])], int(out_lens[k])) for k in range(len(idx))]
        return slots, {"gz_bytes": int(go[-1]), "ms": ist["ms"], "rounds": ist["rounds"]}

    def _scan_layer_slot(self, d_tar, k, opts, contents, window=None, window_lines=None):
        """PrepareLayerTarDevice -> ScanBatchDevice on a tar of k bytes in HBM: (ScanArgs list, walk dict, [types.Secret])"""
        p_dst, offs, scan_paths, binf, walk, _ms = self.PrepareLayerTarDevice(d_tar, k, **opts)
        kw = {} if window_lines is None else {"window_lines": window_lines}
        secrets = self.ScanBatchDevice(p_dst, offs, scan_paths, binf, window=window, **kw)
        data = p_dst[:int(offs[-1])].cpu().numpy().tobytes() if contents and len(scan_paths) else None
        args = [ScanArgs(p, data[int(offs[j]):int(offs[j + 1])] if data is not None else (b"" if contents else None),
                         bool(binf[j])) for j, p in enumerate(scan_paths)]
        return args, walk, secrets

    def InflateZstdDevice(self, d_z, z_offsets, caps=None, bounds=None, max_regrow=9, with_stats=False):
        """A batch of zstd streams that lies in HBM, decoded there
        (tsg_inflate_zstd_device): what layer.Uncompressed() does to a layer
        that starts 28 b5 2f fd, for all such layers at once, one wavefront per
        stream.

        d_z, z_offsets: as InflateGzipDevice's d_gz, gz_offsets.  caps: each
        stream's slot size; default bounds + 64 rounded up to 16 bytes, where
        bounds is tsg_zstd_size_bound of every stream (the caller's, taken
        from the blobs before the upload; else the streams are read back from
        d_z once to walk their headers).  The decoder lets no block regenerate
        more than Block_Maximum_Size, so the bound holds for every stream the
        walk accepts, and only a caller's own small caps (or a stream whose
        headers are malformed) end in TSG_ZSTD_DST_FULL; such a stream is run
        again in a slot twice as large, at most max_regrow times; only those
        streams run again, the others' outputs are copied on the device.

        Returns (d_dst, dst_offsets, out_lens, status) as InflateGzipDevice
        does, status[i] a TSG_ZSTD_* value (_lib.ZSTD_OK ...; the text:
        tsg_zstd_status_text).  with_stats appends {"ms", "rounds"}."""
        import torch
        L = _lib.lib()
        zo = np.ascontiguousarray(z_offsets, dtype=np.uint64)
        n = len(zo) - 1
        if n < 0:
            raise ValueError("z_offsets must hold at least one entry")
        if d_z.dtype != torch.uint8 or not d_z.is_cuda or not d_z.is_contiguous() or d_z.data_ptr() & 15:
            raise ValueError("d_z must be a contiguous, 16-byte aligned uint8 device tensor")
        if n and d_z.numel() < int(zo[-1]):
            raise ValueError("d_z is shorter than the batch")
        if caps is None:
            if bounds is None:
                host = d_z[:int(zo[-1])].cpu().numpy() if n else np.zeros(0, np.uint8)
                bounds = [self.ZstdSizeBound(host[int(zo[i]):int(zo[i + 1])])[0] for i in range(n)]
            caps = np.asarray(bounds, np.int64) + 64
        caps = (np.asarray(caps, np.int64) + 15) & ~15 if n else np.zeros(0, np.int64)
        if len(caps) != n:
            raise ValueError("caps must hold one entry per stream")
        status = np.full(n, _lib.ZSTD_DST_FULL, np.int32)
        out_lens = np.zeros(n, np.uint64)
        dst, do, ms, rounds = None, None, 0.0, 0
        torch.cuda.current_stream(d_z.device).synchronize()      # the call runs on its own stream
        while True:
            new_do = np.zeros(n + 1, np.uint64)
            np.cumsum(caps, out=new_do[1:])
            new = torch.empty(max(int(new_do[-1]), 16) + 16, dtype=torch.uint8, device=d_z.device)
            todo = np.flatnonzero(status == _lib.ZSTD_DST_FULL)
            if dst is not None:                  # what is done moves over on the device
                for i in np.flatnonzero(status != _lib.ZSTD_DST_FULL):
                    k = int(out_lens[i])
                    new[int(new_do[i]):int(new_do[i]) + k] = dst[int(do[i]):int(do[i]) + k]
                torch.cuda.current_stream(d_z.device).synchronize()
            dst, do = new, new_do
            runs = np.split(todo, np.flatnonzero(np.diff(todo) != 1) + 1) if len(todo) else []
            for run in runs:                     # adjacent streams go in one launch
                a, b = int(run[0]), int(run[-1]) + 1
                g, d = np.ascontiguousarray(zo[a:b + 1]), np.ascontiguousarray(do[a:b + 1])
                t = ctypes.c_double()
                rc = L.tsg_inflate_zstd_device(self.engine(), ctypes.c_void_p(d_z.data_ptr()), g.ctypes.data, b - a,
                                               ctypes.c_void_p(dst.data_ptr()), d.ctypes.data,
                                               out_lens[a:b].ctypes.data, status[a:b].ctypes.data, ctypes.byref(t))
                if rc != 0 and not L.tsg_last_error().startswith(b"zstd stream "):
                    _lib.check(rc)               # the call itself failed, not a stream
                ms += t.value
            full = status == _lib.ZSTD_DST_FULL
            if not full.any() or rounds >= max_regrow:
                break
            rounds += 1
            caps = np.where(full, caps * 2, caps)
        out = (dst, do, out_lens, status)
        return out + ({"ms": ms, "rounds": rounds},) if with_stats else out

    @staticmethod
    def ZstdSizeBound(blob):
        """tsg_zstd_size_bound of a zstd stream in host memory: (bound, exact,
        clean) -- clean is False when the walk met a malformed or truncated
        header; the bound then covers what precedes it."""
        L = _lib.lib()
        v = np.ascontiguousarray(np.frombuffer(blob, dtype=np.uint8))
        bound, exact = ctypes.c_uint64(), ctypes.c_int()
        rc = L.tsg_zstd_size_bound(v.ctypes.data if len(v) else None, len(v), ctypes.byref(bound), ctypes.byref(exact))
        return int(bound.value), bool(exact.value), rc == 0

    @staticmethod
    def LayerCompression(blob):
        """tsg_layer_compression: _lib.LAYER_NONE / LAYER_GZIP / LAYER_ZSTD by the blob's first bytes."""
        v = np.ascontiguousarray(np.frombuffer(blob, dtype=np.uint8)[:4])
        return int(_lib.lib().tsg_layer_compression(v.ctypes.data if len(v) else None, len(v)))

    def ScanLayersCompressedDevice(self, blobs, skip_files=(), skip_dirs=(), file_patterns=(), config_path="",
                                   with_stats=False, contents=False, window=None, window_lines=None):
        """ScanLayersGzipDevice for layers as layer.Uncompressed() takes them:
        each blob is a gzip stream, a zstd stream or a plain tar, told apart by
        its first bytes (tsg_layer_compression) as go-containerregistry's peek
        does.

            gzip blobs: one upload -> InflateGzipDevice (one launch)
            zstd blobs: one upload -> InflateZstdDevice (one launch)
            plain tars: uploaded as they are
            then per layer, in blob order: PrepareLayerTarDevice -> ScanBatchDevice

        Arguments and the per-layer result are ScanLayersGzipDevice's.  A
        stream that fails raises WalkError with its blob index and the status
        text.  with_stats appends {"gz_bytes", "zstd_bytes", "plain_bytes",
        "tar_bytes", "inflate_ms", "zstd_ms", "inflate_rounds"}.  window,
        window_lines: ScanBatchDevice's, for every layer's scan."""
        if window_lines is not None and window is None:
            raise ValueError("window_lines needs window=(before, after, min_file)")
        L = _lib.lib()
        views = self._blob_views(blobs)
        kinds = [int(L.tsg_layer_compression(v.ctypes.data, min(len(v), 4))) if len(v) else _lib.LAYER_NONE for v in views]
        opts = dict(skip_files=skip_files, skip_dirs=skip_dirs, file_patterns=file_patterns, config_path=config_path)
        slots = [None] * len(views)              # per blob: (device tensor that holds the tar, its length)
        stats = {"gz_bytes": 0, "zstd_bytes": 0, "plain_bytes": 0, "tar_bytes": 0, "inflate_ms": 0.0, "zstd_ms": 0.0,
                 "inflate_rounds": 0}
        gz = [i for i, k in enumerate(kinds) if k == _lib.LAYER_GZIP]
        zs = [i for i, k in enumerate(kinds) if k == _lib.LAYER_ZSTD]
        plain = [i for i, k in enumerate(kinds) if k == _lib.LAYER_NONE]
        if gz:
            got, st = self._gzip_layer_slots(views, gz)
            for i, slot in zip(gz, got):
                slots[i] = slot
            stats["gz_bytes"], stats["inflate_ms"] = st["gz_bytes"], st["ms"]
            stats["inflate_rounds"] += st["rounds"]
        if zs:
            bounds = [self.ZstdSizeBound(views[i])[0] for i in zs]
            d_z, zo = self._upload_blobs(views, zs)
            dst, do, out_lens, status, ist = self.InflateZstdDevice(d_z, zo, bounds=bounds, with_stats=True)
            for k, i in enumerate(zs):
                if status[k] != _lib.ZSTD_OK:
                    text = L.tsg_zstd_status_text(int(status[k])).decode() or "the decoded layer does not fit its slot"
                    raise WalkError("layer %d: %s" % (i, text))
                slots[i] = (dst[int(do[k]):int(do[k + 1])], int(out_lens[k]))
            stats["zstd_bytes"], stats["zstd_ms"] = int(zo[-1]), ist["ms"]
            stats["inflate_rounds"] += ist["rounds"]
        if plain:                                # one upload for all of them, every tar 16-byte aligned
            d_p, po = self._upload_blobs(views, plain, align=16)
            for k, i in enumerate(plain):
                slots[i] = (d_p[int(po[k]):int(po[k + 1]) + (16 if k == len(plain) - 1 else 0)], len(views[i]))
                stats["plain_bytes"] += len(views[i])
        layers = [self._scan_layer_slot(d_tar, k, opts, contents, window, window_lines) for d_tar, k in slots]
        stats["tar_bytes"] = sum(k for _, k in slots)
        return (layers, stats) if with_stats else layers

    def ScanLayerGzipDevice(self, blob, **kw):
        """ScanLayersGzipDevice for one layer: (ScanArgs list, walk dict, [types.Secret])."""
        kw.pop("with_stats", None)
        return self.ScanLayersGzipDevice([blob], **kw)[0]

    def Scan(self, args):
        return self.ScanBatch([args])[0]

    def ScanBatchResult(self, args_list):
        """ScanBatch keeping the C result object (trivy_amd.report.ScanResult),
        for report assembly (trivy_amd.report.JSONReport)."""
        from .report import ScanResult
        data, offsets = pack(args_list)
        paths, lens, _keep = _lib.pack_paths([a.FilePath for a in args_list])
        binary = np.array([1 if a.Binary else 0 for a in args_list] or [0], dtype=np.uint8)
        res = ctypes.c_void_p()
        _lib.check(_lib.lib().tsg_scan_batch(self.engine(), data.ctypes.data, offsets.ctypes.data,
                                             len(args_list), paths, lens, binary.ctypes.data,
                                             ctypes.byref(res)))
        return ScanResult(res)

    def ScanBatch(self, args_list, with_stats=False):
        data, offsets = pack(args_list)
        paths, lens, _keep = _lib.pack_paths([a.FilePath for a in args_list])
        binary = np.array([1 if a.Binary else 0 for a in args_list] or [0], dtype=np.uint8)
        res = ctypes.c_void_p()
        _lib.check(_lib.lib().tsg_scan_batch(self.engine(), data.ctypes.data, offsets.ctypes.data,
                                             len(args_list), paths, lens, binary.ctypes.data,
                                             ctypes.byref(res)))
        try:
            out = _lib.result_json(res)
            stats = _lib.result_stats(res)
        finally:
            _lib.lib().tsg_result_free(res)
        for s in out:
            s.pop("Error", None)
        return (out, stats) if with_stats else out

    def _scan_device_tensor(self, d_data, offsets, paths, binary, h_data, with_stats, window=None, window_lines=None):
        """tsg_scan_batch_device (h_data None) or tsg_scan_batch_resident on a
        uint8 device tensor; returns (findings, stats or None, C result)."""
        import torch
        L = _lib.lib()
        off = np.ascontiguousarray(offsets, dtype=np.uint64)
        nfiles = len(off) - 1
        if nfiles != len(paths):
            raise ValueError("offsets must hold one more entry than paths")
        total = int(off[-1]) if nfiles else 0
        if d_data.dtype != torch.uint8 or not d_data.is_cuda or not d_data.is_contiguous():
            raise ValueError("d_data must be a contiguous uint8 device tensor")
        if d_data.numel() < total + 16 or d_data.data_ptr() % 16:
            raise ValueError("d_data must be 16-byte aligned and hold 16 bytes past the batch")
        cpaths, lens, _keep = _lib.pack_paths(paths)
        b = np.ascontiguousarray(binary if binary is not None else np.zeros(max(nfiles, 1)), dtype=np.uint8)
        torch.cuda.current_stream(d_data.device).synchronize()     # the engine runs on its own streams
        res = ctypes.c_void_p()
        if window_lines is not None and (h_data is not None or window is None):
            raise ValueError("window_lines needs window=(before, after, min_file)")
        if window_lines is not None:
            opts = _lib.scan_opts2(window, window_lines)
            _lib.check(L.tsg_scan_batch_device_opts2(self.engine(), ctypes.c_void_p(d_data.data_ptr()), off.ctypes.data,
                                                     nfiles, cpaths, lens, b.ctypes.data, ctypes.byref(opts),
                                                     ctypes.byref(res)))
        elif h_data is None and window is not None:
            opts = _lib.scan_opts(window)
            _lib.check(L.tsg_scan_batch_device_opts(self.engine(), ctypes.c_void_p(d_data.data_ptr()), off.ctypes.data,
                                                    nfiles, cpaths, lens, b.ctypes.data, ctypes.byref(opts),
                                                    ctypes.byref(res)))
        elif h_data is None:
            _lib.check(L.tsg_scan_batch_device(self.engine(), ctypes.c_void_p(d_data.data_ptr()), off.ctypes.data,
                                               nfiles, cpaths, lens, b.ctypes.data, ctypes.byref(res)))
        else:
            h = np.ascontiguousarray(h_data, dtype=np.uint8)
            if len(h) < total:
                raise ValueError("h_data is shorter than the batch")
            _lib.check(L.tsg_scan_batch_resident(self.engine(), ctypes.c_void_p(d_data.data_ptr()), h.ctypes.data,
                                                 off.ctypes.data, nfiles, cpaths, lens, b.ctypes.data,
                                                 ctypes.byref(res)))
        try:
            out = _lib.result_json(res)
            stats = None
            if with_stats:
                stats = _lib.result_stats(res)
                stats.update(_lib.result_gather_stats(res))
                stats.update(_lib.result_gather_window_stats(res))
                stats.update(_lib.result_gather_line_stats(res))
        finally:
            L.tsg_result_free(res)
        for s in out:
            s.pop("Error", None)
        return (out, stats) if with_stats else out

    def ScanBatchDevice(self, d_data, offsets, paths, binary=None, with_stats=False, window=None, window_lines=None):
        """The device-only scan (tsg_scan_batch_device): the batch exists only
        in HBM.  d_data: uint8 device tensor, the files packed back to back,
        16-byte aligned, with at least 16 bytes after the batch; offsets:
        nfiles + 1 host integers (0 ... total); paths: the files' FilePath;
        binary: optional per-file flags.  After its second pass the GPU
        gathers the files the exact confirmer reads into host memory; nothing
        else of the batch crosses the link.  The caller's stream is
        synchronised first.  with_stats adds the scan's stats and the gather's
        (gather_files, gather_bytes, gather_runs, gather_ms, gather_retries).

        window = (before, after, min_file) (tsg_scan_batch_device_opts): files
        of at least min_file bytes whose candidates the confirmer decides from
        their starts alone contribute only the bytes [s - before, s + after)
        around each candidate start s (and their first chunk), not the whole
        file; a file whose confirmation would read past what was gathered is
        fetched whole at the end of the call.  The findings are the same for
        every setting.  with_stats then also holds window_files, window_runs,
        window_bytes, fallback_files and fallback_bytes
        (tsg_result_gather_window_stats); gather_bytes counts everything that
        crossed.  None, or before = after = 0: whole files.

        window_lines = cap (tsg_scan_batch_device_opts2, with window only):
        each window grows to the lines the confirmer reads -- back to the
        start of the line two above the candidate, on to the end of the line
        below the match -- found on the GPU from the bytes and K1's newline
        counts, each walk at most cap bytes long.  Small before / after then
        do for every file whose lines are shorter than the cap.  with_stats
        adds line_widened, line_capped and line_ms
        (tsg_result_gather_line_stats).  0: the byte windows alone.

        The chain for files uploaded as read, of any kind (CRLF text, binaries
        to drop, binary .pyc files), is PrepareBatchDevice -> ScanBatchDevice,
        the device twin of PrepareBatch -> ScanBatch:

            dst, off, scan_paths, index, binary, _ = sc.PrepareBatchDevice(d_raw, raw_offsets, paths)
            found = sc.ScanBatchDevice(dst, off, scan_paths, binary)

        -- found[k] belongs to paths[index[k]]; the prepared bytes stay on the
        device, only offsets and flags come back.  For a batch known to be all
        text, StripCR alone does the content preparation:

            dst, new_off, total, _ = sc.StripCR(d_raw, d_raw_offsets, nfiles, raw_total)
            found = sc.ScanBatchDevice(dst, new_off.cpu().numpy(), paths)"""
        if window_lines is not None and window is None:
            raise ValueError("window_lines needs window=(before, after, min_file)")
        return self._scan_device_tensor(d_data, offsets, paths, binary, None, with_stats, window, window_lines)

    def ScanBatchResident(self, d_data, h_data, offsets, paths, binary=None, with_stats=False):
        """tsg_scan_batch_resident: as ScanBatchDevice, with the caller's host
        copy h_data (uint8 array of the batch) for the confirmer instead of
        the GPU's gather."""
        return self._scan_device_tensor(d_data, offsets, paths, binary, h_data, with_stats)


NewScanner = Scanner


def pack(args_list):
    """Pack contents back to back: (uint8 data padded by 64 B, uint64 offsets)."""
    lens = np.fromiter((len(a.Content) for a in args_list), dtype=np.uint64, count=len(args_list))
    offsets = np.zeros(len(args_list) + 1, dtype=np.uint64)
    np.cumsum(lens, out=offsets[1:])
    data = np.zeros(int(offsets[-1]) + 64, dtype=np.uint8)
    for a, o in zip(args_list, offsets[:-1]):
        if len(a.Content):
            data[int(o):int(o) + len(a.Content)] = np.frombuffer(a.Content, dtype=np.uint8)
    return data, offsets


def PrepareBatch(scanner, files, config_path="", image=False, threads=0, file_patterns=()):
    """Batched SecretAnalyzer.Required + Analyze content prep (tsg_prepare_batch;
    pkg/fanal/analyzer/secret/secret.go:103-190).  files: [(input.FilePath, raw
    bytes)].  Returns (ScanArgs list, source index list) for the kept files;
    image=True adds the "/" prefix image files get (secret.go:133-135).
    file_patterns: --file-patterns entries (tsg_prepare_batch_opts): a
    "secret:<re>" match bypasses Required (analyzer.go:417-419)."""
    L = _lib.lib()
    raw, offsets = pack([ScanArgs(p, c) for p, c in files])
    paths, lens, _keep = _lib.pack_paths([p for p, _ in files])
    h = ctypes.c_void_p()
    if file_patterns:
        o, keep = _lib.feed_opts(config_path, file_patterns, threads=threads)
        rc = L.tsg_prepare_batch_opts(scanner._rs, raw.ctypes.data, offsets.ctypes.data, len(files), paths, lens,
                                      ctypes.byref(o), ctypes.byref(h))
        if rc != 0:
            raise ConfigError(L.tsg_last_error().decode("utf-8", "replace"))
    else:
        _lib.check(L.tsg_prepare_batch(scanner._rs, (config_path or "").encode(), raw.ctypes.data,
                                       offsets.ctypes.data, len(files), paths, lens, threads, ctypes.byref(h)))
    try:
        d, o, ix, b = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
        nk = ctypes.c_uint32()
        _lib.check(L.tsg_prepared_view(h, ctypes.byref(d), ctypes.byref(o), ctypes.byref(ix), ctypes.byref(b),
                                       ctypes.byref(nk)))
        n = nk.value
        offs = np.ctypeslib.as_array(ctypes.cast(o, ctypes.POINTER(ctypes.c_uint64)), shape=(n + 1,)).copy() \
            if n else np.zeros(1, np.uint64)
        idx = np.ctypeslib.as_array(ctypes.cast(ix, ctypes.POINTER(ctypes.c_uint32)), shape=(n,)).tolist() if n else []
        binf = np.ctypeslib.as_array(ctypes.cast(b, ctypes.POINTER(ctypes.c_uint8)), shape=(n,)).tolist() if n else []
        data = ctypes.string_at(d, int(offs[-1])) if n else b""
    finally:
        L.tsg_prepared_free(h)
    out = []
    for k, i in enumerate(idx):
        p = files[i][0]
        out.append(ScanArgs("/" + p if image else p, data[int(offs[k]):int(offs[k + 1])], bool(binf[k])))
    return out, idx


class WalkError(Exception):
    """walker.LayerTar.Walk's error ("failed to extract the archive: ...")."""


def PrepareLayerTar(scanner, tar, skip_files=(), skip_dirs=(), config_path="", threads=0, pinned=False,
                    scan=False):
    """One container layer: walker.LayerTar.Walk (pkg/fanal/walker/tar.go:35-103)
    over the uncompressed layer tar `tar` (bytes), then SecretAnalyzer.Required
    + Analyze content prep for every regular file (tsg_prepare_layer_tar).
    Returns (ScanArgs list with "/"-prefixed image paths, walk dict with
    "files", "opq_dirs", "wh_files").  scan=True also runs the prepared batch
    through tsg_scan_batch straight from the prepared (pinned when `pinned`)
    buffer and returns (ScanArgs list, walk dict, [types.Secret]); scan="result"
    returns a report.ScanResult in place of the list."""
    L = _lib.lib()
    buf = np.frombuffer(tar, dtype=np.uint8) if len(tar) else np.zeros(1, np.uint8)
    sf = [s.encode() for s in skip_files]
    sd = [s.encode() for s in skip_dirs]
    sfa = (ctypes.c_char_p * max(1, len(sf)))(*sf)
    sda = (ctypes.c_char_p * max(1, len(sd)))(*sd)
    h = ctypes.c_void_p()
    rc = L.tsg_prepare_layer_tar(scanner._rs, (config_path or "").encode(), buf.ctypes.data, len(tar), sfa, len(sf),
                                 sda, len(sd), threads, 1 if pinned else 0, ctypes.byref(h))
    if rc != 0:
        raise WalkError(L.tsg_last_error().decode("utf-8", "replace"))
    try:
        walk = json.loads(L.tsg_prepared_walk_json(h).decode("utf-8", "surrogateescape"))
        d, o, ix, b = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
        nk = ctypes.c_uint32()
        _lib.check(L.tsg_prepared_view(h, ctypes.byref(d), ctypes.byref(o), ctypes.byref(ix), ctypes.byref(b),
                                       ctypes.byref(nk)))
        n = nk.value
        pp, pl = ctypes.POINTER(ctypes.c_char_p)(), ctypes.POINTER(ctypes.c_uint32)()
        _lib.check(L.tsg_prepared_paths(h, ctypes.byref(pp), ctypes.byref(pl)))
        offs = np.ctypeslib.as_array(ctypes.cast(o, ctypes.POINTER(ctypes.c_uint64)), shape=(n + 1,)).copy() \
            if n else np.zeros(1, np.uint64)
        binf = np.ctypeslib.as_array(ctypes.cast(b, ctypes.POINTER(ctypes.c_uint8)), shape=(n,)).tolist() if n else []
        data = ctypes.string_at(d, int(offs[-1])) if n else b""
        out = [ScanArgs(ctypes.string_at(pp[k], pl[k]).decode("utf-8", "surrogateescape"),
                        data[int(offs[k]):int(offs[k + 1])], bool(binf[k])) for k in range(n)]
        if not scan:
            return out, walk
        res = ctypes.c_void_p()
        _lib.check(L.tsg_scan_batch(scanner.engine(), d, o, n, pp, ctypes.cast(pl, ctypes.c_void_p), b, ctypes.byref(res)))
        if scan == "result":                 # the C result object, for report assembly
            from .report import ScanResult
            return out, walk, ScanResult(res)
        try:
            secrets = _lib.result_json(res)
        finally:
            L.tsg_result_free(res)
        return out, walk, secrets
    finally:
        L.tsg_prepared_free(h)


def _prepared_view(L, h):
    """(offsets uint64 array, index list, binary list, bytes or None) of a
    tsg_prepared handle; the bytes are None for a device preparation."""
    d, o, ix, b = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
    nk = ctypes.c_uint32()
    _lib.check(L.tsg_prepared_view(h, ctypes.byref(d), ctypes.byref(o), ctypes.byref(ix), ctypes.byref(b),
                                   ctypes.byref(nk)))
    n = nk.value
    offs = np.ctypeslib.as_array(ctypes.cast(o, ctypes.POINTER(ctypes.c_uint64)), shape=(n + 1,)).copy()
    idx = np.ctypeslib.as_array(ctypes.cast(ix, ctypes.POINTER(ctypes.c_uint32)), shape=(n,)).tolist() if n else []
    binf = np.ctypeslib.as_array(ctypes.cast(b, ctypes.POINTER(ctypes.c_uint8)), shape=(n,)).tolist() if n else []
    data = ctypes.string_at(d, int(offs[-1])) if d.value else None
    return offs, idx, binf, data


def prepare_batch_view(scanner, files, config_path="", file_patterns=(), model=False):
    """tsg_prepare_batch_opts (model=False) or the CPU model of the device
    preparation, tsg_prepare_device_model (model=True), on files = [(path,
    raw bytes)] as plain arrays: {"offsets", "index", "binary", "data"}; the
    model adds "kinds" (per raw file) and "new_offsets" (nfiles + 1).  Tests."""
    L = _lib.lib()
    raw, offsets = pack([ScanArgs(p, c) for p, c in files])
    paths, lens, _keep = _lib.pack_paths([p for p, _ in files])
    o, keep = _lib.feed_opts(config_path, file_patterns)
    h = ctypes.c_void_p()
    out = {}
    if model:
        kinds = np.zeros(max(len(files), 1), np.uint8)
        new_off = np.zeros(len(files) + 1, np.uint64)
        _lib.check(L.tsg_prepare_device_model(scanner._rs, raw.ctypes.data, offsets.ctypes.data, len(files), paths,
                                              lens, ctypes.byref(o), kinds.ctypes.data, new_off.ctypes.data,
                                              ctypes.byref(h)))
        out["kinds"] = kinds[:len(files)].tolist()
        out["new_offsets"] = new_off
    else:
        _lib.check(L.tsg_prepare_batch_opts(scanner._rs, raw.ctypes.data, offsets.ctypes.data, len(files), paths,
                                            lens, ctypes.byref(o), ctypes.byref(h)))
    del keep
    try:
        out["offsets"], out["index"], out["binary"], out["data"] = _prepared_view(L, h)
    finally:
        L.tsg_prepared_free(h)
    return out


def prepare_print_table():
    """The device preparation's printable table: 256 values of 0 / 1 (test hook)."""
    t = (ctypes.c_uint8 * 256)()
    _lib.check(_lib.lib().tsg_prepare_print_table(t))
    return list(t)


def _prepared_args(L, h, with_paths, paths_in=None):
    """(ScanArgs list, walk dict or None) of a tsg_prepared handle."""
    d, o, ix, b = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
    nk = ctypes.c_uint32()
    _lib.check(L.tsg_prepared_view(h, ctypes.byref(d), ctypes.byref(o), ctypes.byref(ix), ctypes.byref(b),
                                   ctypes.byref(nk)))
    n = nk.value
    offs = np.ctypeslib.as_array(ctypes.cast(o, ctypes.POINTER(ctypes.c_uint64)), shape=(n + 1,)).copy() \
        if n else np.zeros(1, np.uint64)
    binf = np.ctypeslib.as_array(ctypes.cast(b, ctypes.POINTER(ctypes.c_uint8)), shape=(n,)).tolist() if n else []
    index = np.ctypeslib.as_array(ctypes.cast(ix, ctypes.POINTER(ctypes.c_uint32)), shape=(n,)).tolist() if n else []
    data = ctypes.string_at(d, int(offs[-1])) if n else b""
    if with_paths:
        pp, pl = ctypes.POINTER(ctypes.c_char_p)(), ctypes.POINTER(ctypes.c_uint32)()
        _lib.check(L.tsg_prepared_paths(h, ctypes.byref(pp), ctypes.byref(pl)))
        names = [ctypes.string_at(pp[k], pl[k]).decode("utf-8", "surrogateescape") for k in range(n)]
    else:
        names = [paths_in[i] for i in index]
    return [ScanArgs(names[k], data[int(offs[k]):int(offs[k + 1])], bool(binf[k])) for k in range(n)], (d, o, b, n)


def PrepareFsTree(scanner, root, skip_files=(), skip_dirs=(), file_patterns=(), config_path="", threads=0,
                  pinned=False, scan=False):
    """`trivy fs ROOT` feed: walker.FS.Walk + AnalyzeFile's gate + reads + content
    prep (tsg_prepare_fs_tree).  Returns (ScanArgs list, walk dict); scan=True
    also scans the prepared batch through tsg_scan_batch and returns
    (ScanArgs list, walk dict, [types.Secret])."""
    L = _lib.lib()
    o, keep = _lib.feed_opts(config_path, file_patterns, skip_files, skip_dirs, threads, pinned)
    h = ctypes.c_void_p()
    rc = L.tsg_prepare_fs_tree(scanner._rs, os.fsencode(root), ctypes.byref(o), ctypes.byref(h))
    if rc != 0:
        raise WalkError(L.tsg_last_error().decode("utf-8", "replace"))
    try:
        walk = json.loads(L.tsg_prepared_walk_json(h).decode("utf-8", "surrogateescape"))
        args, (d, off, b, n) = _prepared_args(L, h, True)
        if not scan:
            return args, walk
        pp, pl = ctypes.POINTER(ctypes.c_char_p)(), ctypes.POINTER(ctypes.c_uint32)()
        _lib.check(L.tsg_prepared_paths(h, ctypes.byref(pp), ctypes.byref(pl)))
        res = ctypes.c_void_p()
        _lib.check(L.tsg_scan_batch(scanner.engine(), d, off, n, pp, ctypes.cast(pl, ctypes.c_void_p), b,
                                    ctypes.byref(res)))
        try:
            secrets = _lib.result_json(res)
        finally:
            L.tsg_result_free(res)
        return args, walk, secrets
    finally:
        L.tsg_prepared_free(h)


def _reader(fileobj):
    """A tsg_read_fn over a Python binary file object (io.Reader): readinto()
    straight into the engine's buffer where the object has it (one copy),
    else read() + memmove."""
    into = [getattr(fileobj, "readinto", None)]

    def read(_user, buf, cap):
        try:
            if into[0] is not None:
                try:
                    n = into[0](memoryview((ctypes.c_char * cap).from_address(buf)).cast("B"))
                    return n or 0
                except NotImplementedError:    # io.RawIOBase subclasses with read() only
                    into[0] = None
            b = fileobj.read(cap)
        except Exception:                      # noqa: BLE001 -- a reader error ends the walk
            return -1
        if not b:
            return 0
        ctypes.memmove(buf, b, len(b))
        return len(b)
    return _lib.READ_FN(read)


class _Walk(collections.abc.Mapping):
    """Walk's outcome ("files", "opq_dirs", "wh_files", "stats"), decoded from
    the engine's JSON on first use (a layer's walked-path list runs to
    megabytes; most callers only want the findings)."""

    def __init__(self, raw):
        self._raw, self._d = raw, None

    def _get(self):
        if self._d is None:
            self._d = json.loads(self._raw.decode("utf-8", "surrogateescape")) if self._raw else {}
            self._raw = None
        return self._d

    def __getitem__(self, k):
        return self._get()[k]

    def __iter__(self):
        return iter(self._get())

    def __len__(self):
        return len(self._get())


def _stream_result(L, rc, res, as_result):
    if rc != 0:
        raise WalkError(L.tsg_last_error().decode("utf-8", "replace"))
    walk = _Walk(L.tsg_result_walk_json(res))
    if as_result:
        from .report import ScanResult
        return ScanResult(res), walk
    try:
        secrets = _lib.result_json(res)
    finally:
        L.tsg_result_free(res)
    for sec in secrets:
        sec.pop("Error", None)
    return secrets, walk


def ScanLayerStream(scanner, fileobj, skip_files=(), skip_dirs=(), file_patterns=(), config_path="", threads=0,
                    batch_bytes=0, as_result=False, model=False):
    """One container layer read from a binary file object in order (an
    io.Reader): walker.LayerTar.Walk -> AnalyzeFile's gate -> Analyze's prep ->
    Scan, in bounded batches scanned while the next one is read
    (tsg_scan_layer_stream).  Returns ([types.Secret] of every scanned file in
    walk order, walk dict with "files", "opq_dirs", "wh_files", "stats");
    as_result=True gives a report.ScanResult in place of the list.
    model=True runs the CPU model of the GPU passes (tests)."""
    L = _lib.lib()
    o, keep = _lib.feed_opts(config_path, file_patterns, skip_files, skip_dirs, threads)
    cb = _reader(fileobj)
    res = ctypes.c_void_p()
    if model:
        rc = L.tsg_scan_layer_stream_model(scanner._rs, cb, None, ctypes.byref(o), batch_bytes, ctypes.byref(res))
    else:
        rc = L.tsg_scan_layer_stream(scanner.engine(), cb, None, ctypes.byref(o), batch_bytes, ctypes.byref(res))
    return _stream_result(L, rc, res, as_result)


def ScanFsTree(scanner, root, skip_files=(), skip_dirs=(), file_patterns=(), config_path="", threads=0,
               batch_bytes=0, as_result=False, model=False):
    """`trivy fs ROOT` streamed (tsg_scan_fs_tree): the walk and gate of
    PrepareFsTree, the kept files read in walk order in bounded batches, each
    scanned while the next is read.  Returns ([types.Secret], walk dict)."""
    L = _lib.lib()
    o, keep = _lib.feed_opts(config_path, file_patterns, skip_files, skip_dirs, threads)
    res = ctypes.c_void_p()
    if model:
        rc = L.tsg_scan_fs_tree_model(scanner._rs, os.fsencode(root), ctypes.byref(o), batch_bytes, ctypes.byref(res))
    else:
        rc = L.tsg_scan_fs_tree(scanner.engine(), os.fsencode(root), ctypes.byref(o), batch_bytes, ctypes.byref(res))
    return _stream_result(L, rc, res, as_result)


# ScanQueue::kPeakHold (queue.h): a peak of concurrent callers not seen
# again for this long is over
QUEUE_PEAK_HOLD_S = 0.010


class ScanQueue:
    """Per-file Scanner.Scan for unchanged callers (tsg_queue_*): concurrent
    Scan calls (SecretAnalyzer.Analyze, secret.go:137, from --parallel
    goroutines) share one engine batch."""

    def __init__(self, scanner, max_files=0, max_bytes=0, max_wait_us=200, max_inflight=0, model=False,
                 fail_path=None):
        """model=True (tests only): the CPU model of the GPU passes as the
        batch stage (tsg_queue_create_model), no GPU needed; a batch holding
        `fail_path` then fails with an injected bad_alloc."""
        self._sc = scanner
        self._q = ctypes.c_void_p()
        if model:
            fp = fail_path.encode("utf-8", "surrogateescape") if fail_path else None
            _lib.check(_lib.lib().tsg_queue_create_model(scanner._rs, max_files, max_bytes, max_wait_us,
                                                         max_inflight, fp, ctypes.byref(self._q)))
        else:
            _lib.check(_lib.lib().tsg_queue_create(scanner.engine(), max_files, max_bytes, max_wait_us,
                                                   max_inflight, ctypes.byref(self._q)))

    def Scan(self, args):
        L = _lib.lib()
        p = args.FilePath.encode("utf-8", "surrogateescape")
        c = args.Content
        buf = (ctypes.c_char * max(1, len(c))).from_buffer_copy(c) if c else None
        res = ctypes.c_void_p()
        _lib.check(L.tsg_queue_scan(self._q, p, len(p), buf, len(c), 1 if args.Binary else 0, ctypes.byref(res)))
        try:
            out = _lib.result_json(res)[0]
        finally:
            L.tsg_result_free(res)
        out.pop("Error", None)
        return out

    def stats(self):
        v = [ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint32()]
        _lib.check(_lib.lib().tsg_queue_stats(self._q, *[ctypes.byref(x) for x in v]))
        t = ctypes.c_uint64()
        _lib.check(_lib.lib().tsg_queue_timeouts(self._q, ctypes.byref(t)))
        return {"calls": v[0].value, "batches": v[1].value, "files": v[2].value, "max_batch": v[3].value,
                "timeouts": t.value}

    def probe(self, args_list, callers):
        """callers threads scanning args_list file by file through the queue
        (tsg_queue_probe); returns (seconds, findings)."""
        data, offsets = pack(args_list)
        paths, lens, _keep = _lib.pack_paths([a.FilePath for a in args_list])
        sec, nf = ctypes.c_double(), ctypes.c_uint64()
        _lib.check(_lib.lib().tsg_queue_probe(self._q, data.ctypes.data, offsets.ctypes.data, len(args_list), paths,
                                              lens, callers, ctypes.byref(sec), ctypes.byref(nf)))
        return sec.value, nf.value

    def close(self):
        if self._q:
            _lib.lib().tsg_queue_destroy(self._q)
            self._q = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---------------------------------------------------------------- test hooks
def scan_host_reference(scanner, args_list, threads=1):
    """The C++ confirmer on every (file, rule) pair, no prefilter (tests only)."""
    data, offsets = pack(args_list)
    paths, lens, _keep = _lib.pack_paths([a.FilePath for a in args_list])
    binary = np.array([1 if a.Binary else 0 for a in args_list] or [0], dtype=np.uint8)
    res = ctypes.c_void_p()
    _lib.check(_lib.lib().tsg_scan_host_reference(scanner._rs, data.ctypes.data, offsets.ctypes.data,
                                                  len(args_list), paths, lens, binary.ctypes.data, threads,
                                                  ctypes.byref(res)))
    try:
        out = _lib.result_json(res)
    finally:
        _lib.lib().tsg_result_free(res)
    for s in out:
        s.pop("Error", None)
    return out


def scan_host_reference_result(scanner, args_list, threads=1):
    """scan_host_reference keeping the C result object (tests only)."""
    from .report import ScanResult
    data, offsets = pack(args_list)
    paths, lens, _keep = _lib.pack_paths([a.FilePath for a in args_list])
    binary = np.array([1 if a.Binary else 0 for a in args_list] or [0], dtype=np.uint8)
    res = ctypes.c_void_p()
    _lib.check(_lib.lib().tsg_scan_host_reference(scanner._rs, data.ctypes.data, offsets.ctypes.data,
                                                  len(args_list), paths, lens, binary.ctypes.data, threads,
                                                  ctypes.byref(res)))
    return ScanResult(res)


def scan_table_model(scanner, args_list):
    """CPU model of the compiled GPU tables feeding the confirmer (tests only)."""
    data, offsets = pack(args_list)
    paths, lens, _keep = _lib.pack_paths([a.FilePath for a in args_list])
    binary = np.array([1 if a.Binary else 0 for a in args_list] or [0], dtype=np.uint8)
    res = ctypes.c_void_p()
    _lib.check(_lib.lib().tsg_scan_table_model(scanner._rs, data.ctypes.data, offsets.ctypes.data,
                                               len(args_list), paths, lens, binary.ctypes.data,
                                               ctypes.byref(res)))
    try:
        out = _lib.result_json(res)
    finally:
        _lib.lib().tsg_result_free(res)
    for s in out:
        s.pop("Error", None)
    return out


def _result_candidates(res):
    """{(file, rule): sorted np.uint64 starts} of a result's non-empty
    candidate lists (tsg_result_candidate_keys + tsg_result_candidates)."""
    L = _lib.lib()
    kp, kn = ctypes.c_void_p(), ctypes.c_size_t()
    _lib.check(L.tsg_result_candidate_keys(res, ctypes.byref(kp), ctypes.byref(kn)))
    try:
        keys = np.ctypeslib.as_array(ctypes.cast(kp, ctypes.POINTER(ctypes.c_uint32)),
                                     shape=(kn.value, 2)).copy() if kn.value else np.zeros((0, 2), np.uint32)
    finally:
        L.tsg_free(kp)
    out = {}
    p, n = ctypes.c_void_p(), ctypes.c_size_t()
    for f, r in keys.tolist():
        _lib.check(L.tsg_result_candidates(res, f, r, ctypes.byref(p), ctypes.byref(n)))
        out[(f, r)] = np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ctypes.c_uint64)), shape=(n.value,)).copy()
    return out


def _result_file_flags(res):
    L = _lib.lib()
    p, n = ctypes.c_void_p(), ctypes.c_size_t()
    _lib.check(L.tsg_result_file_flags(res, ctypes.byref(p), ctypes.byref(n)))
    if not n.value:
        return np.zeros(0, np.uint32)
    return np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ctypes.c_uint32)), shape=(n.value,)).copy()


FILE_FOLD_SPECIAL = 1      # TSG_FILE_FOLD_SPECIAL (trivy_secret_test.h)
FULL_SCAN_START = np.uint64(0xFFFFFFFFFFFFFFFF)    # kFullScanStart (prefilter.h)


def prefilter_table_model(scanner, args_list, with_info=False):
    """CPU model of K1 + K2 alone on the packed batch (tsg_prefilter_table_model):
    {(file, rule): np.uint64 starts}; with_info adds {"special": one bool per
    file, "hits": anchor hits, "candidates": distinct candidates}.  Tests only."""
    data, offsets = pack(args_list)
    res = ctypes.c_void_p()
    _lib.check(_lib.lib().tsg_prefilter_table_model(scanner._rs, data.ctypes.data, offsets.ctypes.data,
                                                    len(args_list), ctypes.byref(res)))
    try:
        cands = _result_candidates(res)
        st = _lib.result_stats(res)
        special = (_result_file_flags(res) & FILE_FOLD_SPECIAL) != 0
    finally:
        _lib.lib().tsg_result_free(res)
    if not with_info:
        return cands
    return cands, {"special": special, "hits": st["hits"], "candidates": st["candidates"]}


def table_model_candidates(scanner, args_list):
    """The candidates tsg_scan_table_model planned its confirmation from: the
    base tables' for a file without fold-special runes, the variant tables'
    for one with them.  Tests only."""
    data, offsets = pack(args_list)
    paths, lens, _keep = _lib.pack_paths([a.FilePath for a in args_list])
    binary = np.array([1 if a.Binary else 0 for a in args_list] or [0], dtype=np.uint8)
    res = ctypes.c_void_p()
    _lib.check(_lib.lib().tsg_scan_table_model(scanner._rs, data.ctypes.data, offsets.ctypes.data,
                                               len(args_list), paths, lens, binary.ctypes.data,
                                               ctypes.byref(res)))
    try:
        return _result_candidates(res)
    finally:
        _lib.lib().tsg_result_free(res)


def prefilter_resident(scanner, args_list, pad=None, device="cuda:0"):
    """K1 + K2 on the GPU over the packed batch, uploaded with torch
    (tsg_prefilter_resident): ({(file, rule): np.uint64 starts}, info) with
    info = {"chunk_newlines": np.uint16 per K1 chunk, "chunk_bytes", "flags":
    np.uint32 per file, "stats"}.  pad: up to 64 bytes that follow the batch in
    device memory in place of zeros (the kernels may read them, never use
    them).  Tests only."""
    import torch
    L = _lib.lib()
    data, offsets = pack(args_list)
    if pad:
        total = int(offsets[-1])
        data[total:total + len(pad[:64])] = np.frombuffer(pad[:64], dtype=np.uint8)
    d = torch.from_numpy(data).to(device)
    torch.cuda.synchronize()
    res = ctypes.c_void_p()
    _lib.check(L.tsg_prefilter_resident(scanner.engine(), ctypes.c_void_p(d.data_ptr()), data.ctypes.data,
                                        offsets.ctypes.data, len(args_list), ctypes.byref(res)))
    try:
        cands = _result_candidates(res)
        p, n, ch = ctypes.c_void_p(), ctypes.c_size_t(), ctypes.c_uint32()
        _lib.check(L.tsg_result_chunk_newlines(res, ctypes.byref(p), ctypes.byref(n), ctypes.byref(ch)))
        nl = np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ctypes.c_uint16)), shape=(n.value,)).copy() \
            if n.value else np.zeros(0, np.uint16)
        info = {"chunk_newlines": nl, "chunk_bytes": ch.value, "flags": _result_file_flags(res),
                "stats": _lib.result_stats(res)}
    finally:
        L.tsg_result_free(res)
    del d
    return cands, info


def scan_raw(scanner, args_list, resident=False, base=0, pinned=True, data_shift=0, device="cuda:0"):
    """tsg_scan_batch (or, resident, tsg_scan_batch_resident) with the raw-output
    hook on (tsg_test_keep_raw; it stays on for the scanner's engine): the real
    Engine::scan with its cuts, upload ring, wire feed, direct stage, leads and
    pooled lanes.  Returns (findings, {(file, rule): np.uint64 starts}, info)
    with info = {"flags": np.uint32 per file, "segments": one dict per segment
    (f0, nfiles, lead, b0, bytes, lead_bytes, chunk_bytes, hits, lead_flags,
    lead_emitted, "chunk_newlines": np.uint16 per chunk, "lead_cands":
    [(rule, start)]), "stats"}.

    Upload: the batch lies data_shift bytes into a tsg_alloc_pinned buffer
    (pinned) or a numpy array (pageable).  resident: it lies `base` bytes (a
    multiple of 16) above a 256-byte boundary of device memory, uploaded with
    torch; the host copy the confirmer needs is the packed array.  Tests only."""
    L = _lib.lib()
    data, offsets = pack(args_list)
    n = len(data)
    paths, lens, _keep = _lib.pack_paths([a.FilePath for a in args_list])
    binary = np.array([1 if a.Binary else 0 for a in args_list] or [0], dtype=np.uint8)
    eng = scanner.engine()
    _lib.check(L.tsg_test_keep_raw(eng, 1))
    res = ctypes.c_void_p()
    pin = ctypes.c_void_p()
    d = None
    try:
        if resident:
            import torch
            full = torch.zeros(base + n + 256, dtype=torch.uint8, device=device)
            if full.data_ptr() % 256 != 0 or base % 16 != 0:
                raise ValueError("scan_raw: device allocation or base is not aligned")
            d = full[base:base + n]
            d.copy_(torch.from_numpy(data))
            torch.cuda.synchronize()
            _lib.check(L.tsg_scan_batch_resident(eng, ctypes.c_void_p(d.data_ptr()), data.ctypes.data,
                                                 offsets.ctypes.data, len(args_list), paths, lens, binary.ctypes.data,
                                                 ctypes.byref(res)))
        else:
            if pinned:
                _lib.check(L.tsg_alloc_pinned(n + data_shift, ctypes.byref(pin)))
                host = np.ctypeslib.as_array(ctypes.cast(pin, ctypes.POINTER(ctypes.c_uint8)), shape=(n + data_shift,))
            else:
                host = np.zeros(n + data_shift, np.uint8)
            host[:data_shift] = 0x41
            host[data_shift:] = data
            _lib.check(L.tsg_scan_batch(eng, host.ctypes.data + data_shift, offsets.ctypes.data, len(args_list), paths,
                                        lens, binary.ctypes.data, ctypes.byref(res)))
        findings = _lib.result_json(res)
        for s in findings:
            s.pop("Error", None)
        ns = ctypes.c_size_t()
        _lib.check(L.tsg_result_raw_segments(res, ctypes.byref(ns)))
        segs = []
        for k in range(ns.value):
            rec = _lib.TsgRawSegment()
            _lib.check(L.tsg_result_raw_segment(res, k, ctypes.byref(rec)))
            sd = {f: getattr(rec, f) for f in ("f0", "nfiles", "lead", "chunk_bytes", "b0", "bytes", "lead_bytes", "hits",
                                               "lead_flags", "lead_emitted")}

            def arr(p, ctype, dtype, count):
                if not count:
                    return np.zeros(0, dtype)
                return np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ctype)), shape=(count,)).copy()
            sd["chunk_newlines"] = arr(rec.chunk_newlines, ctypes.c_uint16, np.uint16, rec.nchunks)
            sd["lead_cands"] = list(zip(arr(rec.lead_cand_rules, ctypes.c_uint32, np.uint32, rec.nlead_cands).tolist(),
                                        arr(rec.lead_cand_starts, ctypes.c_uint64, np.uint64, rec.nlead_cands).tolist()))
            segs.append(sd)
        info = {"flags": _result_file_flags(res), "segments": segs, "stats": _lib.result_stats(res)}
        return findings, _result_candidates(res), info
    finally:
        if res:
            L.tsg_result_free(res)
        if pin:
            L.tsg_free_pinned(pin)
        del d


def plan_gather(offsets, need, chunk, lead=0):
    """The device-only scan's gather layout (tsg_test_plan_gather, csrc/gather.h):
    (goff np.uint64 per file, runs np.uint64 [nruns, 3] of (source, destination,
    length), total).  Tests only."""
    off = np.ascontiguousarray(offsets, dtype=np.uint64)
    nd = np.ascontiguousarray(need, dtype=np.uint8)
    nfiles = len(off) - 1
    goff = np.zeros(max(nfiles, 1), np.uint64)
    runs = np.zeros((nfiles // 2 + 2, 3), np.uint64)
    nruns, total = ctypes.c_size_t(), ctypes.c_uint64()
    _lib.check(_lib.lib().tsg_test_plan_gather(off.ctypes.data, nfiles, lead, nd.ctypes.data, chunk, goff.ctypes.data,
                                                runs.ctypes.data, len(runs), ctypes.byref(nruns),
                                                ctypes.byref(total)))
    return goff[:nfiles], runs[:nruns.value].copy(), total.value


def plan_gather_windows(offsets, cands, fflags, all_rules, windowable, chunk, window, lead=0):
    """The windowed gather layout (tsg_test_plan_gather_windows, csrc/gather.h
    plan_gather_windows): cands = [(file, rule, start)]; returns a dict of cls,
    first_run, marks, runs [nruns, 3], total.  Tests only."""
    off = np.ascontiguousarray(offsets, dtype=np.uint64)
    nfiles = len(off) - 1
    cf = np.array([c[0] for c in cands] or [0], np.uint32)
    cr = np.array([c[1] for c in cands] or [0], np.uint32)
    cs = np.array([c[2] for c in cands] or [0], np.uint64)
    ff = np.ascontiguousarray(fflags if len(fflags) else [0], dtype=np.uint32)
    wr = np.ascontiguousarray(windowable if len(windowable) else [0], dtype=np.uint8)
    nchunks = (int(off[-1]) + chunk - 1) // chunk if nfiles else 0
    cls = np.zeros(max(nfiles, 1), np.uint8)
    first = np.zeros(max(nfiles, 1), np.uint32)
    marks = np.zeros(max(nchunks, 1), np.uint8)
    runs = np.zeros((nchunks // 2 + 2, 3), np.uint64)
    nruns, total = ctypes.c_size_t(), ctypes.c_uint64()
    opts = _lib.scan_opts(window)
    _lib.check(_lib.lib().tsg_test_plan_gather_windows(
        off.ctypes.data, nfiles, lead, cf.ctypes.data, cr.ctypes.data, cs.ctypes.data, len(cands), ff.ctypes.data,
        1 if all_rules else 0, wr.ctypes.data, len(windowable), chunk, ctypes.byref(opts), cls.ctypes.data,
        first.ctypes.data, marks.ctypes.data, runs.ctypes.data, len(runs), ctypes.byref(nruns), ctypes.byref(total)))
    return {"cls": cls[:nfiles], "first_run": first[:nfiles], "marks": marks[:nchunks],
            "runs": runs[:nruns.value].copy(), "total": total.value}


def plan_gather_lines(data, offsets, cands, fflags, all_rules, windowable, chunk, window, window_lines, lead=0):
    """plan_gather_windows with a line cap (tsg_test_plan_gather_lines, csrc/gather.h
    line_window on the frame's bytes `data`): the same dict plus "widened" and
    "capped".  window_lines 0: plan_gather_windows' layout.  Tests only."""
    off = np.ascontiguousarray(offsets, dtype=np.uint64)
    nfiles = len(off) - 1
    total_bytes = int(off[-1]) if nfiles else 0
    d = np.frombuffer(bytes(data[:total_bytes]) or b"\0", dtype=np.uint8).copy() if not isinstance(data, np.ndarray) \
        else np.ascontiguousarray(data, dtype=np.uint8)
    if len(d) < total_bytes:
        raise ValueError("data is shorter than the offsets say")
    cf = np.array([c[0] for c in cands] or [0], np.uint32)
    cr = np.array([c[1] for c in cands] or [0], np.uint32)
    cs = np.array([c[2] for c in cands] or [0], np.uint64)
    ff = np.ascontiguousarray(fflags if len(fflags) else [0], dtype=np.uint32)
    wr = np.ascontiguousarray(windowable if len(windowable) else [0], dtype=np.uint8)
    nchunks = (total_bytes + chunk - 1) // chunk
    cls = np.zeros(max(nfiles, 1), np.uint8)
    first = np.zeros(max(nfiles, 1), np.uint32)
    marks = np.zeros(max(nchunks, 1), np.uint8)
    runs = np.zeros((nchunks // 2 + 2, 3), np.uint64)
    nruns, total = ctypes.c_size_t(), ctypes.c_uint64()
    widened, capped = ctypes.c_uint64(), ctypes.c_uint64()
    opts = _lib.scan_opts2(window, window_lines)
    _lib.check(_lib.lib().tsg_test_plan_gather_lines(
        d.ctypes.data, off.ctypes.data, nfiles, lead, cf.ctypes.data, cr.ctypes.data, cs.ctypes.data, len(cands),
        ff.ctypes.data, 1 if all_rules else 0, wr.ctypes.data, len(windowable), chunk, ctypes.byref(opts),
        cls.ctypes.data, first.ctypes.data, marks.ctypes.data, runs.ctypes.data, len(runs), ctypes.byref(nruns),
        ctypes.byref(total), ctypes.byref(widened), ctypes.byref(capped)))
    return {"cls": cls[:nfiles], "first_run": first[:nfiles], "marks": marks[:nchunks],
            "runs": runs[:nruns.value].copy(), "total": total.value, "widened": widened.value, "capped": capped.value}


def windowable_rows(scanner):
    """(one byte per row of the rule table, number of rules) (tsg_test_windowable_rows).  Tests only."""
    n, nr = ctypes.c_size_t(), ctypes.c_size_t()
    _lib.check(_lib.lib().tsg_test_windowable_rows(scanner._rs, None, 0, ctypes.byref(n), ctypes.byref(nr)))
    rows = np.zeros(max(n.value, 1), np.uint8)
    _lib.check(_lib.lib().tsg_test_windowable_rows(scanner._rs, rows.ctypes.data, n.value, ctypes.byref(n), ctypes.byref(nr)))
    return rows[:n.value], nr.value


def regex_examined(pattern, text, pos, submatch=False, cut=None):
    """(match end or -1, furthest byte index examined) of the anchored run of
    pattern at text[pos] on text[:cut] (tsg_test_regex_examined).  Tests only."""
    t = np.frombuffer(bytes(text[:cut] if cut is not None else text) or b"\0", dtype=np.uint8).copy()
    n = len(text[:cut] if cut is not None else text)
    end, ex = ctypes.c_long(), ctypes.c_size_t()
    _lib.check(_lib.lib().tsg_test_regex_examined(pattern.encode(), t.ctypes.data, n, pos, 1 if submatch else 0,
                                                  ctypes.byref(end), ctypes.byref(ex)))
    return end.value, ex.value


def _window_segment(res, k):
    """Segment k's window record (tsg_result_window_segment): classes and insufficient files."""
    rec = _lib.TsgWindowSegment()
    _lib.check(_lib.lib().tsg_result_window_segment(res, k, ctypes.byref(rec)))

    def arr(p, ctype, dtype, count):
        if not count:
            return np.zeros(0, dtype)
        return np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ctype)), shape=(count,)).copy()
    return {"cls": arr(rec.cls, ctypes.c_uint8, np.uint8, rec.nfiles),
            "insufficient": arr(rec.insufficient, ctypes.c_uint32, np.uint32, rec.ninsufficient).tolist()}


def scan_device_model_windows(scanner, args_list, chunk, window, window_lines=None):
    """CPU model of the device-only scan with windows (tsg_scan_device_model_opts;
    with window_lines, a line cap, tsg_scan_device_model_opts2):
    (findings, gather record of the windowed round with "cls" and
    "insufficient", gather record of the fallback round, stats).  Tests only."""
    data, offsets = pack(args_list)
    paths, lens, _keep = _lib.pack_paths([a.FilePath for a in args_list])
    binary = np.array([1 if a.Binary else 0 for a in args_list] or [0], dtype=np.uint8)
    res = ctypes.c_void_p()
    if window_lines is not None:
        opts = _lib.scan_opts2(window, window_lines)
        _lib.check(_lib.lib().tsg_scan_device_model_opts2(scanner._rs, data.ctypes.data, offsets.ctypes.data,
                                                          len(args_list), paths, lens, binary.ctypes.data, chunk,
                                                          ctypes.byref(opts), None, None, ctypes.byref(res)))
    else:
        opts = _lib.scan_opts(window)
        _lib.check(_lib.lib().tsg_scan_device_model_opts(scanner._rs, data.ctypes.data, offsets.ctypes.data,
                                                         len(args_list), paths, lens, binary.ctypes.data, chunk,
                                                         ctypes.byref(opts), None, None, ctypes.byref(res)))
    try:
        out = _lib.result_json(res)
        for s in out:
            s.pop("Error", None)
        rec = _gather_segment(res, 0)
        rec.update(_window_segment(res, 0))
        stats = _lib.result_gather_stats(res)
        stats.update(_lib.result_gather_window_stats(res))
        if window_lines is not None:
            stats.update(_lib.result_gather_line_stats(res))
        ns = ctypes.c_size_t()
        _lib.check(_lib.lib().tsg_result_raw_segments(res, ctypes.byref(ns)))
        return out, rec, _gather_segment(res, 1) if ns.value > 1 else None, stats
    finally:
        _lib.lib().tsg_result_free(res)


def _gather_segment(res, k):
    """Segment k's gather record of a result (tsg_result_gather_segment) as a dict."""
    rec = _lib.TsgGatherSegment()
    _lib.check(_lib.lib().tsg_result_gather_segment(res, k, ctypes.byref(rec)))

    def arr(p, ctype, dtype, count):
        if not count:
            return np.zeros(0, dtype)
        return np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ctype)), shape=(count,)).copy()
    return {"nfiles": rec.nfiles, "total": rec.total,
            "need": arr(rec.need, ctypes.c_uint8, np.uint8, rec.nfiles if rec.need else 0),
            "goff": arr(rec.goff, ctypes.c_uint64, np.uint64, rec.nfiles),
            "runs": arr(rec.runs, ctypes.c_uint64, np.uint64, 3 * rec.nruns).reshape(-1, 3),
            "caps": arr(rec.caps, ctypes.c_uint64, np.uint64, rec.ncaps).tolist(),
            "guard_ok": arr(rec.guard_ok, ctypes.c_uint8, np.uint8, rec.ncaps).tolist(),
            "bytes": arr(rec.bytes, ctypes.c_uint8, np.uint8, rec.total)}


def scan_device_model(scanner, args_list, chunk, with_gather=False):
    """CPU model of the device-only scan (tsg_scan_device_model): findings, and
    with_gather the gather record and stats.  Tests only."""
    data, offsets = pack(args_list)
    paths, lens, _keep = _lib.pack_paths([a.FilePath for a in args_list])
    binary = np.array([1 if a.Binary else 0 for a in args_list] or [0], dtype=np.uint8)
    res = ctypes.c_void_p()
    _lib.check(_lib.lib().tsg_scan_device_model(scanner._rs, data.ctypes.data, offsets.ctypes.data, len(args_list),
                                                paths, lens, binary.ctypes.data, chunk, ctypes.byref(res)))
    try:
        out = _lib.result_json(res)
        for s in out:
            s.pop("Error", None)
        if not with_gather:
            return out
        return out, _gather_segment(res, 0), _lib.result_gather_stats(res)
    finally:
        _lib.lib().tsg_result_free(res)


def scan_device_raw(scanner, args_list, base=0, pad=16, tail=None, device="cuda:0", window=None, window_lines=None):
    """tsg_scan_batch_device with the raw-output and keep-gather hooks on (they
    stay on for the scanner's engine).  The batch lies `base` bytes (a multiple
    of 16) above a 256-byte boundary of a device tensor that ends `pad` bytes
    after the batch; no host array of the batch is passed to the call.
    Returns (findings, {(file, rule): starts}, info) as scan_raw, each
    info["segments"][k] also holding "gather" (_gather_segment), and
    info["gather_stats"].  window: tsg_scan_batch_device_opts' windows; each
    segment's "gather" then also holds "cls" and "insufficient",
    info["gather_stats"] the window stats and info["fallback"] the fallback
    round's gather record over the batch (None: no file fell back).
    window_lines: the line cap (tsg_scan_batch_device_opts2); the line stats
    then join info["gather_stats"].  Tests only."""
    import torch
    L = _lib.lib()
    data, offsets = pack(args_list)
    total = int(offsets[-1])
    paths, lens, _keep = _lib.pack_paths([a.FilePath for a in args_list])
    binary = np.array([1 if a.Binary else 0 for a in args_list] or [0], dtype=np.uint8)
    eng = scanner.engine()
    _lib.check(L.tsg_test_keep_raw(eng, 1))
    _lib.check(L.tsg_test_keep_gather(eng, 1))
    full = torch.zeros(base + total + pad, dtype=torch.uint8, device=device)
    if full.data_ptr() % 256 != 0 or base % 16 != 0 or pad < 16:
        raise ValueError("scan_device_raw: device allocation, base or pad is not as required")
    host = data[:total + pad].copy()
    if tail is not None:
        host[total:] = np.frombuffer((tail * pad)[:pad], dtype=np.uint8)
    full[base:].copy_(torch.from_numpy(host))
    torch.cuda.synchronize()
    res = ctypes.c_void_p()
    try:
        if window_lines is not None:
            opts = _lib.scan_opts2(window, window_lines)
            _lib.check(L.tsg_scan_batch_device_opts2(eng, ctypes.c_void_p(full.data_ptr() + base), offsets.ctypes.data,
                                                     len(args_list), paths, lens, binary.ctypes.data, ctypes.byref(opts),
                                                     ctypes.byref(res)))
        elif window is not None:
            opts = _lib.scan_opts(window)
            _lib.check(L.tsg_scan_batch_device_opts(eng, ctypes.c_void_p(full.data_ptr() + base), offsets.ctypes.data,
                                                    len(args_list), paths, lens, binary.ctypes.data, ctypes.byref(opts),
                                                    ctypes.byref(res)))
        else:
            _lib.check(L.tsg_scan_batch_device(eng, ctypes.c_void_p(full.data_ptr() + base), offsets.ctypes.data,
                                               len(args_list), paths, lens, binary.ctypes.data, ctypes.byref(res)))
        findings = _lib.result_json(res)
        for s in findings:
            s.pop("Error", None)
        ns = ctypes.c_size_t()
        _lib.check(L.tsg_result_raw_segments(res, ctypes.byref(ns)))
        segs = []
        wst = _lib.result_gather_window_stats(res) if window is not None else None
        nseg = ns.value - (1 if wst and wst["fallback_files"] else 0)   # (the fallback round's record follows the segments')
        for k in range(nseg):
            rec = _lib.TsgRawSegment()
            _lib.check(L.tsg_result_raw_segment(res, k, ctypes.byref(rec)))
            sd = {f: getattr(rec, f) for f in ("f0", "nfiles", "lead", "chunk_bytes", "b0", "bytes", "lead_bytes")}
            sd["gather"] = _gather_segment(res, k)
            if window is not None:
                sd["gather"].update(_window_segment(res, k))
            segs.append(sd)
        info = {"flags": _result_file_flags(res), "segments": segs, "stats": _lib.result_stats(res),
                "gather_stats": _lib.result_gather_stats(res)}
        if window is not None:
            info["gather_stats"].update(wst)
            if window_lines is not None:
                info["gather_stats"].update(_lib.result_gather_line_stats(res))
            info["fallback"] = _gather_segment(res, nseg) if nseg < ns.value else None
        return findings, _result_candidates(res), info
    finally:
        if res:
            L.tsg_result_free(res)
        del full


def prefilter_device_gather(scanner, args_list, device="cuda:0"):
    """The two GPU passes and the device-only scan's gather on one resident
    segment, without a confirmation (tsg_prefilter_resident with h_data NULL and
    the keep-gather hook on): ({(file, rule): starts}, info) with info as
    scan_device_raw's.  Tests only."""
    import torch
    L = _lib.lib()
    data, offsets = pack(args_list)
    eng = scanner.engine()
    _lib.check(L.tsg_test_keep_gather(eng, 1))
    d = torch.from_numpy(data).to(device)
    torch.cuda.synchronize()
    res = ctypes.c_void_p()
    _lib.check(L.tsg_prefilter_resident(eng, ctypes.c_void_p(d.data_ptr()), None, offsets.ctypes.data, len(args_list),
                                        ctypes.byref(res)))
    try:
        st = _lib.result_stats(res)
        seg = {"f0": 0, "nfiles": len(args_list), "lead": 0, "chunk_bytes": st["chunk_bytes"], "b0": 0,
               "bytes": int(offsets[-1]), "lead_bytes": 0, "gather": _gather_segment(res, 0)}
        info = {"flags": _result_file_flags(res), "segments": [seg], "stats": st,
                "gather_stats": _lib.result_gather_stats(res)}
        return _result_candidates(res), info
    finally:
        L.tsg_result_free(res)
        del d


def gather_pool(scanner):
    """(buffers, idle, bytes) of the engine's gather-buffer pools (tsg_test_gather_pool)."""
    b, i, n = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint64()
    _lib.check(_lib.lib().tsg_test_gather_pool(scanner.engine(), ctypes.byref(b), ctypes.byref(i), ctypes.byref(n)))
    return b.value, i.value, n.value


def plan_segments(offsets, resident=False, base=0, with_paths=True, **policy):
    """The engine's segment planner on an offsets array (tsg_test_plan_segments):
    one dict per segment (f0, nfiles with the lead, lead, b0, bytes, d_data) plus
    "lead_bytes".  policy: every field of tsg_segment_policy.  Tests only."""
    off = np.ascontiguousarray(offsets, dtype=np.uint64)
    nfiles = len(off) - 1
    pol = _lib.TsgSegmentPolicy(**policy)
    cap = max(nfiles, 1)
    out = (_lib.TsgSegmentInfo * cap)()
    nout = ctypes.c_uint32()
    reb = np.zeros(nfiles + 2 * cap + 2, np.uint64)
    _lib.check(_lib.lib().tsg_test_plan_segments(off.ctypes.data, nfiles, int(resident), base, int(with_paths),
                                                  ctypes.byref(pol), out, cap, ctypes.byref(nout), reb.ctypes.data,
                                                  len(reb)))
    segs, r = [], 0
    for s in out[:nout.value]:
        sd = {k: getattr(s, k) for k, _ in s._fields_}
        sd["lead_bytes"] = int(reb[r + 1]) if s.lead else 0
        r += s.nfiles + 1
        segs.append(sd)
    return segs


def k1_schedule(nchunks, blocks, rounds=1, top8=False, with_items=True):
    """K1's item schedule as the host restates it (tsg_test_k1_schedule,
    csrc/k1_schedule.h) for nchunks chunks on `blocks` workgroups: {"n8", "n4",
    "n2", "n1": chunks per level, "nitems", "grid_ok", "W": blocks * 16, and
    with_items "kU", "c0", "rend": np.uint64 arrays, one entry per item}.
    Tests only."""
    L = _lib.lib()
    lv = np.zeros(6, np.uint64)
    _lib.check(L.tsg_test_k1_schedule(nchunks, blocks, rounds, int(top8), lv.ctypes.data, None, 0))
    out = {"n8": int(lv[0]), "n4": int(lv[1]), "n2": int(lv[2]), "n1": int(lv[3]), "nitems": int(lv[4]),
           "grid_ok": bool(lv[5]), "W": 16 * blocks}
    if with_items:
        items = np.zeros((max(out["nitems"], 1), 3), np.uint64)
        _lib.check(L.tsg_test_k1_schedule(nchunks, blocks, rounds, int(top8), lv.ctypes.data, items.ctypes.data,
                                          len(items)))
        items = items[:out["nitems"]].astype(np.int64)
        out["kU"], out["c0"], out["rend"] = items[:, 0].copy(), items[:, 1].copy(), items[:, 2].copy()
    return out


def prefilter_report(scanner):
    buf = ctypes.c_void_p()
    _lib.check(_lib.lib().tsg_prefilter_report(scanner._rs, ctypes.byref(buf)))
    try:
        return ctypes.string_at(buf).decode("utf-8", "replace")
    finally:
        _lib.lib().tsg_free(buf)
