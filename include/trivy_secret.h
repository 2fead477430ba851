/*
 * trivy_secret.h -- C-ABI of the MI355X-native secret-scanning engine
 * (drop-in for mmorel-35/trivy pkg/fanal/secret).
 *
 * Reference interface each entry point replaces (paths relative to the
 * reference repository):
 *
 *   tsg_ruleset_compile     secret.ParseConfig + secret.NewScanner
 *                           pkg/fanal/secret/scanner.go:277-307, 320-364
 *   tsg_ruleset_allow_path  (Global).AllowPath        scanner.go:56-59
 *   tsg_builtin_rules_json  secret.GetBuiltinRules     builtin-rules.go:87-89
 *   tsg_secret_rules_metadata_json
 *                           secret.GetSecretRulesMetadata builtin-rules.go:91-99
 *   tsg_engine_create       (no reference analogue: binds the compiled
 *                           rules to one GPU; the reference's regexes are
 *                           compiled inside ParseConfig/NewScanner)
 *   tsg_scan_batch          N x (*Scanner).Scan(ScanArgs) -> types.Secret
 *                           scanner.go:366-463, batched as proposed in
 *                           SURVEY.md 8(b); ScanArgs{FilePath, Content,
 *                           Binary} = (paths[i], data[off[i]:off[i+1]],
 *                           binary[i])
 *   tsg_result_*            types.Secret / SecretFinding / Code / Line
 *                           pkg/fanal/types/secret.go:5-20, misconf.go:48-61
 *
 * Test, measurement and tooling hooks (CPU models of the GPU passes, probes of
 * single components, fault injection) are declared in trivy_secret_test.h;
 * the same library exports them, and no product entry point calls them.
 *
 * Conventions
 *   - status: 0 = OK, negative = error; tsg_last_error() returns a
 *     thread-local message for the last failing call on this thread.
 *   - strings crossing the boundary are Go byte strings: pointer + length,
 *     not necessarily valid UTF-8, not NUL-terminated unless stated.
 *   - ownership: the caller owns every input buffer until the call returns;
 *     the library owns every tsg_* object until its *_free/_destroy call.
 *   - threading: a tsg_ruleset is immutable and may be shared.  A tsg_engine
 *     may be shared too: concurrent tsg_scan_batch calls each take their own
 *     lane (compute + copy HIP streams and scratch buffers) on every device
 *     and their own host confirm pool, as the reference's Scan is called
 *     concurrently from --parallel goroutines (analyzer.go:434-451).
 *   - there is no CPU fallback: tsg_engine_create fails with
 *     TSG_ERR_NO_DEVICE when no MI355X (HIP device) is visible.
 */
#ifndef TRIVY_SECRET_H_
#define TRIVY_SECRET_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TSG_OK 0
#define TSG_ERR_INVALID (-1)
#define TSG_ERR_CONFIG (-2)     /* ParseConfig error: yaml/regexp compile error */
#define TSG_ERR_NO_DEVICE (-3)
#define TSG_ERR_HIP (-4)
#define TSG_ERR_INTERNAL (-5)

typedef struct tsg_ruleset tsg_ruleset;
typedef struct tsg_engine tsg_engine;
typedef struct tsg_result tsg_result;

/* One types.Line (misconf.go:51-60). */
typedef struct tsg_line {
  int64_t number;
  const char* content; size_t content_len;
  int32_t is_cause;
  const char* annotation; size_t annotation_len;
  int32_t truncated;
  const char* highlighted; size_t highlighted_len;
  int32_t first_cause;
  int32_t last_cause;
} tsg_line;

/* One types.SecretFinding (secret.go:10-20); Layer is left to the caller. */
typedef struct tsg_finding {
  const char* rule_id; size_t rule_id_len;
  const char* category; size_t category_len;
  const char* severity; size_t severity_len;
  const char* title; size_t title_len;
  int64_t start_line;
  int64_t end_line;
  const char* match; size_t match_len;
  uint32_t num_lines;
} tsg_finding;

typedef struct tsg_stats {
  double k1_ms, k2_ms, h2d_ms, d2h_ms, host_ms, total_ms;
  uint64_t bytes, files, hits, candidates, confirm_files, findings;
  uint32_t k1_blocks, k1_threads, chunk_bytes;
  int32_t table_in_lds;
  double gpu_wall_ms;   /* device driver threads' busy time (sum over devices) */
  uint32_t pieces;      /* pipeline segments the batch was cut into */
  uint32_t k1_launches; /* K1 launches (segments x scan-DFA groups) */
  uint32_t devices;     /* devices that took part */
  double feed_ms;       /* uploaded batches: wall time until the last segment's upload had landed */
  /* wire packing of uploaded batches (text blocks cross the link as 6 or 7 bits per byte) */
  uint64_t wire_bytes;    /* bytes of the batch's data that crossed the link (bytes when nothing went packed) */
  uint32_t packed_strips; /* strips sent packed */
  uint32_t raw_strips;    /* strips sent as they are by the strip feeder */
  double pack_ms;         /* the packer threads' summed busy time */
  /* blocks (4096 bytes) of the strips sent packed, by the mode they crossed in, and the bytes the 6-bit
   * blocks escaped (the 7-bit codec has no 6-bit blocks) */
  uint64_t blocks_6bit;
  uint64_t blocks_7bit;
  uint64_t blocks_raw;
  uint64_t escaped_bytes;
  uint64_t blocks_split;  /* blocks sent in the 6-bit codec's split mode; their escaped bytes count above */
} tsg_stats;

const char* tsg_last_error(void);
const char* tsg_version(void);

/* ParseConfig + NewScanner.  config_json: the trivy-secret.yaml document
 * decoded to JSON with the YAML keys (rules, allow-rules, exclude-block,
 * enable-builtin-rules, disable-rules, disable-allow-rules), or NULL for the
 * builtin rules only (ParseConfig returned nil). */
int tsg_ruleset_compile(const char* config_json, size_t config_len, tsg_ruleset** out);
void tsg_ruleset_free(tsg_ruleset* rs);
int tsg_ruleset_num_rules(const tsg_ruleset* rs);
/* rule id of rule i (NUL-terminated, owned by rs) */
const char* tsg_ruleset_rule_id(const tsg_ruleset* rs, int i);
/* Global.AllowPath(path): 1 allowed, 0 not */
int tsg_ruleset_allow_path(const tsg_ruleset* rs, const char* path, size_t path_len);
/* Compile report of the GPU prefilter (NUL-terminated, owned by the engine). */
const char* tsg_engine_report(const tsg_engine* e);
/* Builtin rule data as JSON (NUL-terminated, static).  GetBuiltinRules,
 * pkg/fanal/secret/builtin-rules.go:87-89. */
const char* tsg_builtin_rules_json(void);
/* GetSecretRulesMetadata (builtin-rules.go:91-99): json.Marshal of the
 * []iacRules.Check{Name: rule ID, Description: rule title} for the builtin
 * rules (NUL-terminated, static). */
const char* tsg_secret_rules_metadata_json(void);

int tsg_device_count(void);
/* device_mask: bit d selects HIP device d (0 = every visible device).  With
 * several devices one tsg_scan_batch call is spread over all of them: the
 * batch is cut into segments (TSG_SEGMENT_BYTES, default 4 GiB) that each
 * device's driver thread pulls from a shared queue. */
int tsg_engine_create(const tsg_ruleset* rs, uint64_t device_mask, tsg_engine** out);
void tsg_engine_destroy(tsg_engine* e);
/* host worker threads for exact confirmation (0 = min(16, hardware)) */
void tsg_engine_set_threads(tsg_engine* e, int threads);

/* Pinned host buffers for the PCIe feed. */
int tsg_alloc_pinned(size_t bytes, void** out);
void tsg_free_pinned(void* p);

/* Scan a batch of nfiles files packed back to back in `data`
 * (offsets[0] = 0, offsets[nfiles] = total bytes).  paths[i] has length
 * path_lens[i] (or is NUL-terminated when path_lens is NULL).  binary may be
 * NULL (all false).  The batch is streamed to HBM in segments (upload of
 * segment k+1 overlapping the kernels of segment k and the host confirmation
 * of segment k-1), scanned by the GPU kernels, and confirmed exactly on the
 * host.  result[i] == Scanner.Scan(args[i]).  `data` should be pinned
 * (tsg_alloc_pinned) for full PCIe rate; pageable memory works, slower. */
int tsg_scan_batch(tsg_engine* e, const uint8_t* data, const uint64_t* offsets, uint32_t nfiles,
                   const char* const* paths, const uint32_t* path_lens, const uint8_t* binary,
                   tsg_result** out);
/* Same, with the batch already resident in HBM at d_data (16-byte aligned,
 * readable for 16 bytes past the end); h_data is the host copy used by the
 * exact confirmer. */
int tsg_scan_batch_resident(tsg_engine* e, const void* d_data, const uint8_t* h_data,
                            const uint64_t* offsets, uint32_t nfiles, const char* const* paths,
                            const uint32_t* path_lens, const uint8_t* binary, tsg_result** out);
/* The device-only scan: the batch exists only in HBM (the output of
 * tsg_strip_cr_device, tsg_inflate_gzip_device, a peer-to-peer read) and no host
 * copy is passed.  d_data: as for tsg_scan_batch_resident (16-byte aligned,
 * readable for 16 bytes past the end, on one of the engine's devices);
 * offsets, paths, path_lens, binary: host arrays as above.  After its second
 * pass the GPU gathers the files the exact confirmer must read -- those with
 * candidates or fold-special content; every file when the rule set has a
 * host-evaluated rule -- into host-mapped memory, and the confirmer runs on
 * that copy: only those files cross the link.  The result is
 * tsg_scan_batch_resident's, byte for byte.  TSG_GATHER_CAP (bytes) sets a
 * gather buffer's first capacity (default: an eighth of a piece + 1 MiB; it
 * grows on demand). */
int tsg_scan_batch_device(tsg_engine* e, const void* d_data, const uint64_t* offsets, uint32_t nfiles,
                          const char* const* paths, const uint32_t* path_lens, const uint8_t* binary,
                          tsg_result** out);
/* The device-only scan gathering windows around candidates instead of whole
 * files: for a batch of large files (logs, dumps, bundles) whose every file
 * has a candidate, the whole batch would otherwise cross the link.  With a
 * window set, a file whose candidates all belong to rules the confirmer
 * decides from a candidate start alone contributes the K1 chunk holding its
 * first byte and, per candidate start s, the chunks of [s - window_before,
 * s + window_after) clipped to the file; chunks that touch form one run.
 * Files stay whole when they are fold-special, when the rule set has a
 * host-evaluated rule, when a candidate belongs to a presence rule, a
 * host-gated keyword rule or an exclude block, when they are shorter than
 * window_min_file, or when their windows take more than half of their chunks.
 * The confirmer works on the runs and notes every read that would leave them
 * on a side that is not the file's own start or end (a regex run that examined
 * a byte at or past its run's end, a line search that met a run's edge, fewer
 * than 4 bytes in front of a candidate); such a file's result is dropped, and
 * at the end of the call those files are gathered whole in one more round and
 * confirmed as tsg_scan_batch_device confirms.  The result is
 * tsg_scan_batch_resident's, byte for byte, for every setting.  opts NULL, or
 * both window sizes 0: tsg_scan_batch_device in every respect.  d_data must
 * stay valid for the whole call. */
typedef struct tsg_device_scan_opts {
  uint32_t window_before;   /* bytes gathered in front of a candidate start; 0 with window_after 0: whole files */
  uint32_t window_after;    /* bytes gathered from a candidate start on */
  uint64_t window_min_file; /* files shorter than this are gathered whole */
} tsg_device_scan_opts;
int tsg_scan_batch_device_opts(tsg_engine* e, const void* d_data, const uint64_t* offsets, uint32_t nfiles,
                               const char* const* paths, const uint32_t* path_lens, const uint8_t* binary,
                               const tsg_device_scan_opts* opts, tsg_result** out);
/* ... with line windows: a window whose size comes from the data.  The
 * confirmer reads lines -- the line of the match, the two above it and the
 * lines below -- so a fixed span fails on every long line.  With
 * window_line_cap != 0 the window of a candidate start s (s < len) of a
 * windowed file of len bytes is [a, b), with t = min(len, s + window_after):
 *   B  the position of the 3rd '\n' met walking back from s - 1 (the
 *      confirmer's line search has to find that byte, so it belongs to the
 *      window), never below max(0, s - window_line_cap); with fewer than 3
 *      there, that lower end;
 *   a  = min(s > window_before ? s - window_before : 0, B);
 *   N  = 2 + the number of '\n' in [s, t);
 *   E  the position just past the N-th '\n' at or after t, never past
 *      min(len, t + window_line_cap); with fewer than N there, that upper end;
 *   b  = max(t, E), and s + 1 at least.
 * The GPU finds the K1 chunks of [a, b) from the bytes at both ends and the
 * newline count it keeps per chunk; everything else -- the head chunk, the
 * files that stay whole, the half-of-the-chunks rule, the fallback round -- is
 * as above, on the widened windows.  A file with a line longer than the cap,
 * or a match longer than window_after, still falls back.  The result is
 * tsg_scan_batch_resident's, byte for byte, for every setting.
 * struct_size: sizeof(tsg_device_scan_opts2) as the caller compiled it (a
 * smaller value than the fields above need is an error).  window_line_cap 0:
 * tsg_scan_batch_device_opts with the same windows, in every respect;
 * window_line_cap != 0 with both window sizes 0 is an error.
 * tsg_scan_batch_device_opts forwards here with cap 0. */
typedef struct tsg_device_scan_opts2 {
  uint32_t struct_size;
  uint32_t window_before;
  uint32_t window_after;
  uint32_t window_line_cap;  /* bytes a line walk may go from s back and from t on; 0: byte windows alone */
  uint64_t window_min_file;
} tsg_device_scan_opts2;
int tsg_scan_batch_device_opts2(tsg_engine* e, const void* d_data, const uint64_t* offsets, uint32_t nfiles,
                                const char* const* paths, const uint32_t* path_lens, const uint8_t* binary,
                                const tsg_device_scan_opts2* opts, tsg_result** out);

/* Host-feed ceiling: stream `bytes` of host memory (pinned for full rate) to
 * HBM through the engine's upload path in segments, with no kernels; *ms =
 * wall time.  Reported beside scan rates, never used by a scan. */
int tsg_feed_probe(tsg_engine* e, const uint8_t* data, uint64_t bytes, double* ms);

/* GPU-side CR strip of a device-resident batch of TEXT files: the analyzer's
 *   content = bytes.ReplaceAll(content, []byte("\r"), []byte(""))
 * (pkg/fanal/analyzer/secret/secret.go:121) for every file at once.  Replaces
 * the host-side strip of tsg_prepare_batch for a feed that uploads files as
 * read.  d_src / d_dst: 16-byte aligned device buffers of >= total bytes on
 * the engine's first device (not overlapping); d_offsets: nfiles + 1 device
 * uint64, nondecreasing, d_offsets[0] = 0, d_offsets[nfiles] = total (checked);
 * d_new_offsets: nfiles + 1 device uint64 receiving each file's start in
 * d_dst.  *out_total = stripped bytes (= d_new_offsets[nfiles]); *ms (may be
 * NULL) = kernel time.  Synchronous.  This is one line of Analyze for a batch
 * the caller knows to be all text; tsg_prepare_batch_device (below) does the
 * whole preparation, binaries included, for a raw batch of any files.  The
 * scan to follow it is tsg_scan_batch_device on
 * d_dst with the host's copy of d_new_offsets (d_dst needs 16 readable bytes
 * past the stripped total): the stripped bytes never leave the device. */
int tsg_strip_cr_device(tsg_engine* e, const void* d_src, const uint64_t* d_offsets, uint32_t nfiles,
                        uint64_t total, void* d_dst, uint64_t* d_new_offsets, uint64_t* out_total, double* ms);

uint32_t tsg_result_num_files(const tsg_result* r);
/* types.Secret.FilePath of file i ("" for types.Secret{}) */
int tsg_result_file_path(const tsg_result* r, uint32_t file, const char** path, size_t* len);
uint32_t tsg_result_num_findings(const tsg_result* r, uint32_t file);
int tsg_result_finding(const tsg_result* r, uint32_t file, uint32_t k, tsg_finding* out);
int tsg_result_line(const tsg_result* r, uint32_t file, uint32_t k, uint32_t line, tsg_line* out);
/* nonzero when the reference would panic on this file (non-participating
 * secret group, scanner.go:155-168 + 465-473) */
int tsg_result_file_error(const tsg_result* r, uint32_t file);
/* Whole result as a JSON array of types.Secret (Go field names); invalid
 * UTF-8 bytes are written as \udcXX escapes.  Free with tsg_free. */
int tsg_result_json(const tsg_result* r, char** json, size_t* len);
int tsg_result_stats(const tsg_result* r, tsg_stats* out);
/* What a tsg_scan_batch_device result's gather took (all 0 for the other
 * scans): files and bytes the GPU placed in host memory for the confirmer,
 * the runs of adjacent files they formed, the gather kernels' time, and copy
 * launches repeated with a larger buffer.  Any pointer may be NULL. */
int tsg_result_gather_stats(const tsg_result* r, uint64_t* files, uint64_t* bytes, uint64_t* runs, double* ms,
                            uint32_t* retries);
/* ... of a tsg_scan_batch_device_opts result with windows (all 0 otherwise):
 * files confirmed from windows, the runs and bytes of the windowed layouts
 * (the whole files in them included), and the files and bytes of the fallback
 * round.  tsg_result_gather_stats' bytes and runs hold both rounds: everything
 * that crossed for the confirmer.  Any pointer may be NULL. */
int tsg_result_gather_window_stats(const tsg_result* r, uint64_t* window_files, uint64_t* window_runs,
                                   uint64_t* window_bytes, uint64_t* fallback_files, uint64_t* fallback_bytes);
/* ... with a line cap (all 0 otherwise): candidates whose line window covers
 * more K1 chunks than their byte window (a repeated candidate counts again),
 * candidates whose walk ended at the cap on either side, and the line pass's
 * own kernel time, which tsg_result_gather_stats' ms includes.  Any pointer
 * may be NULL. */
int tsg_result_gather_line_stats(const tsg_result* r, uint64_t* widened, uint64_t* capped, double* ms);
/* Frees a result; one of >= 4096 files + findings is handed to a background
   thread (its memory returns shortly after the call). */
void tsg_result_free(tsg_result* r);
void tsg_free(void* p);


/* ---- host feed ----
 * Batched SecretAnalyzer.Required + Analyze content preparation, replacing the
 * per-file analyzer calls of pkg/fanal/analyzer/secret/secret.go:103-190
 * (Required: size >= 10, skip dirs/files/exts, the config file itself,
 * global AllowPath; Analyze: utils.IsBinary on the first 300 bytes
 * (utils.go:68-86), binaries other than .pyc dropped, CR stripped from text,
 * ExtractPrintableBytes for .pyc (utils.go:111-143)).  raw/raw_offsets: the
 * files as read; paths: input.FilePath as the analyzer sees it (no "/" prefix
 * for image files: the caller adds it to the scan path, secret.go:133-135).
 * The result packs the kept files back to back (+64 B pad) ready for
 * tsg_scan_batch; index[k] = source file of kept file k. */
typedef struct tsg_prepared tsg_prepared;
int tsg_prepare_batch(const tsg_ruleset* rs, const char* config_path, const uint8_t* raw, const uint64_t* raw_offsets,
                      uint32_t nfiles, const char* const* paths, const uint32_t* path_lens, int threads,
                      tsg_prepared** out);
int tsg_prepared_view(const tsg_prepared* p, const uint8_t** data, const uint64_t** offsets, const uint32_t** index,
                      const uint8_t** binary, uint32_t* nkept);
void tsg_prepared_free(tsg_prepared* p);
/* A container layer: walker.LayerTar.Walk (pkg/fanal/walker/tar.go:35-103)
 * over an uncompressed layer tar in memory -- Go archive/tar's reading of
 * ustar / GNU / PAX headers (long names, PAX path and size), header checksum,
 * TypeRegA normalisation; opaque-directory (".wh..wh..opq") and whiteout
 * (".wh.<name>") entries recorded, not analyzed; skip_files / skip_dirs as
 * walker.Option (utils.CleanSkipPaths + doublestar.Match, utils.go:88-109),
 * files under a skipped directory dropped (underSkippedDir) -- then the same
 * preparation as tsg_prepare_batch for every regular file, with Required
 * seeing the walker's path (no leading '/', analyzer.go:407-408).  pinned != 0
 * packs the kept contents into pinned host memory (tsg_alloc_pinned; heap
 * when no device is present, reported as "pinned": false) so the batch goes
 * to tsg_scan_batch as prepared.  A malformed tar fails with Walk's
 * "failed to extract the archive: ..." error. */
int tsg_prepare_layer_tar(const tsg_ruleset* rs, const char* config_path, const uint8_t* tar, size_t len,
                          const char* const* skip_files, uint32_t nskip_files, const char* const* skip_dirs,
                          uint32_t nskip_dirs, int threads, int pinned, tsg_prepared** out);
/* Analyzer-group options of the secret feed (pkg/fanal/analyzer/analyzer.go
 * AnalyzerOptions / walker.Option):
 *   config_path      SecretAnalyzer.configPath; Required skips its base name;
 *   file_patterns    --file-patterns entries "fileType:regexPattern"
 *                    (analyzer.go:332-350: a malformed entry or regexp fails
 *                    with its error text); "secret:<re>" entries force the
 *                    secret analyzer on matching paths whatever Required says
 *                    (filePatternMatch, analyzer.go:417-419,522-530);
 *   skip_files/dirs  --skip-files / --skip-dirs (walker.Option: doublestar
 *                    patterns; for tsg_prepare_fs_tree made relative to the
 *                    root by BuildSkipPaths, fs.go:99-149);
 *   threads          host threads (0: up to 16); pinned: pack into pinned
 *                    host memory (tsg_alloc_pinned) for tsg_scan_batch. */
typedef struct tsg_feed_opts {
  const char* config_path;
  const char* const* file_patterns;
  uint32_t n_file_patterns;
  const char* const* skip_files;
  uint32_t n_skip_files;
  const char* const* skip_dirs;
  uint32_t n_skip_dirs;
  int32_t threads;
  int32_t pinned;
} tsg_feed_opts;
/* tsg_prepare_batch with feed options (skip lists unused: the files are given). */
int tsg_prepare_batch_opts(const tsg_ruleset* rs, const uint8_t* raw, const uint64_t* raw_offsets, uint32_t nfiles,
                           const char* const* paths, const uint32_t* path_lens, const tsg_feed_opts* opts,
                           tsg_prepared** out);
/* tsg_prepare_batch_opts for a raw batch that lives in HBM: the device twin of
 * tsg_prepare_batch -> tsg_scan_batch is
 *   tsg_prepare_batch_device -> tsg_scan_batch_device,
 * for every kind of file.  d_raw: the files as read, back to back, on one of
 * the engine's devices (read only below raw_offsets[nfiles]); raw_offsets,
 * paths, path_lens: host arrays as for tsg_prepare_batch.  The gate (file
 * patterns, Required) runs on the host from the paths and sizes, on
 * opts->threads threads; of opts only config_path, file_patterns and threads
 * are used (NULL: defaults); the rule set is the engine's.  One device pass
 * then does Analyze's content preparation: IsBinary on every file's first 300
 * bytes, binaries other than .pyc dropped, CR stripped from text,
 * ExtractPrintableBytes for binary .pyc files, the kept contents packed back
 * to back at d_dst followed by 64 zero bytes.  d_raw and d_dst are 16-byte
 * aligned and do not overlap; dst_cap = bytes at d_dst.  The prepared bytes
 * never exceed raw_offsets[nfiles] + (number of .pyc paths), so that + 64
 * always suffices; with less, a batch that does not fit fails with
 * TSG_ERR_INVALID, the size needed in the message and d_dst untouched.
 * *out: an ordinary tsg_prepared whose tsg_prepared_view gives offsets, index,
 * binary and nkept of the kept files and data == NULL (the bytes are at
 * d_dst).  *ms (may be NULL) = kernel time.  Synchronous.  The scan to follow
 * is tsg_scan_batch_device(e, d_dst, offsets, nkept, <kept paths>, ...,
 * binary, ...): nothing of the contents crosses the link before the
 * confirmer's gather. */
int tsg_prepare_batch_device(tsg_engine* e, const void* d_raw, const uint64_t* raw_offsets, uint32_t nfiles,
                             const char* const* paths, const uint32_t* path_lens, const tsg_feed_opts* opts,
                             void* d_dst, uint64_t dst_cap, tsg_prepared** out, double* ms);
/* tsg_prepare_layer_tar with feed options. */
int tsg_prepare_layer_tar_opts(const tsg_ruleset* rs, const uint8_t* tar, size_t len, const tsg_feed_opts* opts,
                               tsg_prepared** out);
/* tsg_prepare_layer_tar_opts for a layer tar that lives in HBM (what
 * tsg_inflate_gzip_device or a peer-to-peer read delivers for an image scan): the first
 * link of
 *   tsg_prepare_layer_tar_device -> tsg_scan_batch_device,
 * walker.LayerTar.Walk (pkg/fanal/walker/tar.go:35-103) included.  d_tar: len
 * bytes on one of the engine's devices (nothing at or past len is read).
 * The walk reads only header blocks, the payload of PAX / GNU long-name
 * entries and the end marker, and every header passes the checksum test: one
 * device pass tests every 512-byte block with it, marks the ones that pass
 * and the payload blocks behind an 'x' / 'g' / 'L' / 'K' one, and stores the
 * marked blocks into host-mapped memory; the walk then runs on the host over
 * them, with archive/tar's semantics unchanged.  Exactness never depends on
 * the marks: a block the walk reads that was not marked is copied from d_tar
 * on its own -- at most two such reads of at most 512 bytes per call (the
 * zero block of the end marker and its successor, or the block at which a
 * malformed tar fails, or a truncated tar's partial tail); a block marked
 * without being a header (a tar stored in the layer) only costs bytes.  The
 * walked files pass the host gate, and the content pass of
 * tsg_prepare_batch_device runs over the tar itself with 2n + 1 interleaved
 * entries -- gap, file 0, gap, file 1, ..., tail gap; a gap (headers,
 * padding, entries not handed on) is dropped -- so d_dst receives
 * tsg_prepare_layer_tar_opts' data byte for byte, followed by 64 zero bytes.
 * Of opts everything but `pinned` is honoured (NULL: defaults); the rule set
 * is the engine's.  d_tar and d_dst are 16-byte aligned and do not overlap;
 * dst_cap = len + 64 always suffices (every file follows a header block that
 * is dropped); with less, a layer that does not fit fails as
 * tsg_prepare_batch_device does (TSG_ERR_INVALID, the size needed in the
 * message, d_dst untouched).  A malformed tar fails with the host call's
 * "failed to extract the archive: ..." text and d_dst untouched; len 0, a len
 * below 512 and zero blocks only behave as on the host.  *out: an ordinary
 * tsg_prepared -- tsg_prepared_view gives data == NULL and the host call's
 * offsets, index and binary, tsg_prepared_paths the "/"-prefixed paths,
 * tsg_prepared_walk_json the same lists with "pinned": false.  *ms (may be
 * NULL) = the content pass's kernel time.  TSG_TAR_GATHER_CAP (bytes) sets
 * the marked blocks' first buffer capacity (default: a sixteenth of the
 * blocks + 1024 blocks); when they do not fit the device pass is repeated
 * with a larger buffer.  Synchronous. */
int tsg_prepare_layer_tar_device(tsg_engine* e, const void* d_tar, uint64_t len, const tsg_feed_opts* opts,
                                 void* d_dst, uint64_t dst_cap, tsg_prepared** out, double* ms);
/* What the device walk of tsg_prepare_layer_tar_device took (any pointer may
 * be NULL): whole 512-byte blocks of the tar, blocks marked, bytes that
 * crossed the link for them, reads served from d_tar because the block was
 * not marked (<= 2), repeats of the device pass after a full buffer, and the
 * mark / count / scan / compact kernels' time in ms (the last repeat's).
 * TSG_ERR_INVALID for a tsg_prepared of another call. */
int tsg_prepared_tar_stats(const tsg_prepared* p, uint64_t* blocks, uint64_t* marked, uint64_t* gathered_bytes,
                           uint32_t* fallback_reads, uint32_t* retries, double* scan_ms);
/* ---- gzip layers inflated on the GPU ----
 * Every layer an image scan receives is a gzip stream, which the reference
 * opens with layer.Uncompressed() (pkg/fanal/artifact/image/image.go:464-492)
 * -- Go's compress/gzip over compress/flate -- before walker.LayerTar.Walk.
 * tsg_inflate_gzip_device is that step for a batch of streams that lies in
 * HBM, and the first link of
 *   tsg_inflate_gzip_device -> tsg_prepare_layer_tar_device -> tsg_scan_batch_device:
 * only the compressed bytes and the confirmer's gather cross the link.
 * Stream i is d_gz[gz_offsets[i], gz_offsets[i + 1]) and inflates into the
 * slot d_dst[dst_offsets[i], dst_offsets[i + 1]); gz_offsets, dst_offsets
 * (nstreams + 1 each, nondecreasing), out_lens and status (nstreams each) are
 * host arrays.  d_gz and d_dst are 16-byte aligned device memory of one
 * device, do not overlap, and every slot starts 16-byte aligned; aligned
 * 16-byte loads may touch up to 16 bytes past d_gz's last stream (the d_data
 * convention above), but nothing past a stream's own end influences its
 * result, and nothing outside a stream's slot is written, whatever the input.
 * One wavefront inflates one stream, the longest streams starting first: the
 * call is parallel across streams, not inside one.  RFC 1952 over RFC 1951
 * as compress/gzip reads it: all members of a stream are inflated one behind
 * the other (multistream), FEXTRA / FNAME / FCOMMENT are skipped, FHCRC and
 * every member's CRC32 and ISIZE are checked; bytes behind the last member
 * are read as another header, so zero padding is an error.  status[i]:
 *   TSG_INFLATE_OK
 *   TSG_INFLATE_HEADER     "gzip: invalid header"
 *   TSG_INFLATE_CORRUPT    "flate: corrupt input" (Go adds an offset; not reproduced)
 *   TSG_INFLATE_EOF        "unexpected EOF"
 *   TSG_INFLATE_CHECKSUM   "gzip: invalid checksum"
 *   TSG_INFLATE_DST_FULL   the output did not fit the slot: call again with a larger one
 * -- the first error in stream order.  out_lens[i] = the bytes written to
 * slot i (for a failed stream, up to where the decoder stopped).  Returns
 * TSG_OK when every stream is TSG_INFLATE_OK, else TSG_ERR_INVALID with the
 * first failing stream's index and text in tsg_last_error(); status[] and
 * out_lens[] are filled either way, and a good stream's output is valid when
 * its neighbour fails.  *ms (may be NULL) = kernel time.  Synchronous; runs
 * on the device that holds d_gz. */
enum {
  TSG_INFLATE_OK = 0,
  TSG_INFLATE_HEADER = 1,
  TSG_INFLATE_CORRUPT = 2,
  TSG_INFLATE_EOF = 3,
  TSG_INFLATE_CHECKSUM = 4,
  TSG_INFLATE_DST_FULL = 5
};
int tsg_inflate_gzip_device(tsg_engine* e, const void* d_gz, const uint64_t* gz_offsets, uint32_t nstreams,
                            void* d_dst, const uint64_t* dst_offsets, uint64_t* out_lens, int32_t* status, double* ms);
/* Go's error text of a status ("" for TSG_INFLATE_OK and TSG_INFLATE_DST_FULL) */
const char* tsg_inflate_status_text(int32_t status);
/* ISIZE of the last member of a gzip stream in host memory: the inflated size
 * mod 2^32 of that member alone -- a hint for the slot's size, no more.
 * TSG_ERR_INVALID when gz does not start like a gzip stream. */
int tsg_gzip_size_hint(const uint8_t* gz, size_t len, uint64_t* isize);
/* ---- zstd layers decoded on the GPU ----
 * layer.Uncompressed() (pkg/fanal/artifact/image/image.go:464-492; at
 * go-containerregistry v0.20.3) peeks a layer's first bytes and unwraps gzip
 * (1f 8b), zstd (28 b5 2f fd; klauspost/compress) or nothing: layers of type
 * application/vnd.oci.image.layer.v1.tar+zstd are what current buildkit and
 * containerd write when asked.  tsg_inflate_zstd_device is that step for a
 * batch of zstd streams that lies in HBM, beside tsg_inflate_gzip_device at
 * the head of the same chain; its arguments, its buffers' rules (alignment, no
 * overlap, the 16-byte-load convention for d_z, nothing outside a slot written
 * and nothing past a stream's end read into its result) and its return values
 * are that call's.  RFC 8878: concatenated and skippable frames; raw, RLE and
 * compressed blocks; raw, RLE, Huffman (one or four streams) and treeless
 * literals; predefined, RLE, FSE and repeat sequence tables; the content
 * checksum (XXH64) and Frame_Content_Size are checked.  Dictionaries are not
 * supported.  One wavefront decodes one stream; a match older than the wave's
 * 32 KiB of LDS history is read back from the slot in HBM.  status[i]:
 *   TSG_ZSTD_OK
 *   TSG_ZSTD_HEADER     bad magic, a reserved bit, an impossible window
 *   TSG_ZSTD_CORRUPT
 *   TSG_ZSTD_EOF        the stream ends inside a frame
 *   TSG_ZSTD_CHECKSUM
 *   TSG_ZSTD_DICT       the frame names a dictionary
 *   TSG_ZSTD_DST_FULL   the output did not fit the slot: call again with a larger one
 * -- the first error in stream order; the statuses and their texts are this
 * library's own (no Go decoder was run against them).  Where a stream both
 * overflows its slot and is malformed further on, the slot comes first. */
enum {
  TSG_ZSTD_OK = 0,
  TSG_ZSTD_HEADER = 1,
  TSG_ZSTD_CORRUPT = 2,
  TSG_ZSTD_EOF = 3,
  TSG_ZSTD_CHECKSUM = 4,
  TSG_ZSTD_DICT = 5,
  TSG_ZSTD_DST_FULL = 6
};
int tsg_inflate_zstd_device(tsg_engine* e, const void* d_z, const uint64_t* z_offsets, uint32_t nstreams,
                            void* d_dst, const uint64_t* dst_offsets, uint64_t* out_lens, int32_t* status, double* ms);
/* The text of a status ("" for TSG_ZSTD_OK and TSG_ZSTD_DST_FULL) */
const char* tsg_zstd_status_text(int32_t status);
/* An upper bound of the decoded size of a zstd stream in host memory, from its
 * frame and block headers alone: the sum of Frame_Content_Size where every
 * frame has one (*exact = 1), else a raw or RLE block counts its size and a
 * compressed block Block_Maximum_Size.  An RLE block expands 128 KiB from
 * four bytes, so no multiple of the compressed size is a bound; this is.
 * TSG_ERR_INVALID when the walk meets a malformed or truncated header; *bound
 * then covers what precedes it. */
int tsg_zstd_size_bound(const uint8_t* z, size_t len, uint64_t* bound, int* exact);
/* How a layer blob is compressed, by its first bytes as go-containerregistry's
 * peek decides: 1f 8b gzip, 28 b5 2f fd zstd, anything else a plain tar. */
enum { TSG_LAYER_NONE = 0, TSG_LAYER_GZIP = 1, TSG_LAYER_ZSTD = 2 };
int tsg_layer_compression(const uint8_t* blob, size_t len);
/* `trivy fs` over a directory tree on disk: walker.FS.Walk (pkg/fanal/walker/
 * fs.go:25-97; filepath.WalkDir order, symlinks not followed, defaultSkipDirs
 * **\/.git proc sys dev, permission errors ignored), AnalyzeFile's gate before
 * a file is opened (analyzer.go:403-419), the kept files read by `threads`
 * readers, then tsg_prepare_batch's preparation.  ScanArgs.FilePath is the
 * walker's path relative to the root (tsg_prepared_paths).  The walk JSON also
 * reports "read_bytes", "walk_ms", "read_ms", "prep_ms". */
int tsg_prepare_fs_tree(const tsg_ruleset* rs, const char* root, const tsg_feed_opts* opts, tsg_prepared** out);
/* The kept files' ScanArgs.FilePath: "/" + the walker's path for a layer tar
 * (image files, secret.go:131-135), the path relative to the root for an fs
 * tree; only for batches made by tsg_prepare_layer_tar* / tsg_prepare_fs_tree. */
int tsg_prepared_paths(const tsg_prepared* p, const char* const** paths, const uint32_t** lens);
/* {"files": [every regular file the walk hands to the analyzers], "opq_dirs":
 * [...], "wh_files": [...], "pinned": bool} (Walk's return values, tar.go:90);
 * owned by p. */
const char* tsg_prepared_walk_json(const tsg_prepared* p);

/* ---- streamed feed -> scan: bounded host memory, the
 * walk / read / prepare of batch k+1 overlapping the scan of batch k.
 * A reader (an io.Reader): > 0 bytes read into buf (at most cap), 0 at the
 * end of the data, < 0 on an error. */
typedef int64_t (*tsg_read_fn)(void* user, uint8_t* buf, size_t cap);
/* One container layer read from `read` in order: walker.LayerTar.Walk over an
 * io.Reader (pkg/fanal/walker/tar.go:35-103) -> AnalyzeFile's gate
 * (analyzer.go:403-419) before a file's content is read -> SecretAnalyzer
 * .Analyze's preparation (secret.go:103-150) -> Scan, the kept files packed
 * into batches of about batch_bytes raw bytes (0: 256 MiB; a larger file is a
 * batch of its own), each scanned on the engine while the next is read.  The
 * result holds every scanned file in walk order, ScanArgs.FilePath = "/" +
 * path; tsg_result_walk_json gives Walk's return values and the feed timing.
 * Layers may be scanned concurrently on one engine (image.go:327's pipeline). */
int tsg_scan_layer_stream(tsg_engine* e, tsg_read_fn read, void* user, const tsg_feed_opts* opts,
                          uint64_t batch_bytes, tsg_result** out);
/* `trivy fs ROOT` streamed: tsg_prepare_fs_tree's walk and gate, the kept files
 * read in walk order in batches of about batch_bytes, each scanned while the
 * next is read.  ScanArgs.FilePath = the path relative to the root. */
int tsg_scan_fs_tree(tsg_engine* e, const char* root, const tsg_feed_opts* opts, uint64_t batch_bytes,
                     tsg_result** out);
/* A streamed result's walk: {"files": [every regular file handed to the
 * analyzers], "opq_dirs": [...], "wh_files": [...], "stats": {wall_ms,
 * feed_ms, scan_ms, wait_ms, walked_bytes, read_bytes, scanned_bytes,
 * batches, files, peak_batch_bytes}}; NULL for other results.  Owned by r. */
const char* tsg_result_walk_json(const tsg_result* r);

/* ---- per-file Scan for unchanged callers ----
 * SecretAnalyzer.Analyze calls Scanner.Scan once per file (pkg/fanal/analyzer/
 * secret/secret.go:137) from --parallel goroutines (analyzer.go:434-451,
 * default 5).  A queue gathers concurrent tsg_queue_scan calls into engine
 * batches: a caller that finds no batch forming leads one, waits until its
 * share of the expected callers has joined -- the recent peak of concurrent
 * callers split over the max_inflight batch slots (default 8), so 5 callers
 * run as 5 concurrent one-file batches and 64 as batches of 8 -- (or
 * max_files / max_bytes is reached, or max_wait_us has passed), scans it,
 * and hands each caller its own result; up to max_inflight batches run at
 * once.  Thread-safe. */
typedef struct tsg_queue tsg_queue;
int tsg_queue_create(tsg_engine* e, uint32_t max_files, uint64_t max_bytes, uint32_t max_wait_us,
                     uint32_t max_inflight, tsg_queue** out);
void tsg_queue_destroy(tsg_queue* q);
/* Scanner.Scan(ScanArgs{path, content, binary}) -> a one-file result */
int tsg_queue_scan(tsg_queue* q, const char* path, size_t path_len, const uint8_t* content, size_t len, int binary,
                   tsg_result** out);
int tsg_queue_stats(tsg_queue* q, uint64_t* calls, uint64_t* batches, uint64_t* files, uint32_t* max_batch);


/* ---- report and image semantics ---- */
typedef struct tsg_layer {          /* ftypes.Layer, pkg/fanal/types/artifact.go:75-79 */
  const char* digest;
  const char* diff_id;
  const char* created_by;
} tsg_layer;

typedef struct tsg_report_opts {
  int64_t schema_version;           /* report.SchemaVersion = 2 (pkg/report/writer.go:24); 0 omits it */
  const char* created_at;           /* CreatedAt, RFC 3339; re-encoded as time.Time marshals */
  const char* artifact_name;        /* ArtifactName; also the Target of image-config secrets */
  const char* artifact_type;        /* artifact.Type: "filesystem", "repository", "container_image", ... */
  const char* metadata_json;        /* types.Metadata as JSON (re-encoded in Go's field order); NULL = zero */
  const char* severities;           /* comma-separated --severity list; NULL = all five */
  int32_t layers_sorted;            /* 1: layers are cached blobs (AnalysisResult.Sort already applied) */
} tsg_report_opts;

/* `trivy -f json` output (pkg/report/json.go:22-50) for the secret results of
 * one artifact.  layers[i] = tsg_scan_batch results of layer i, lowest layer
 * first (an fs scan is one layer, layer_refs may be NULL); per layer
 * AnalysisResult.Sort (analyzer.go:224-235), across layers ApplyLayers'
 * mergeSecrets (applier/docker.go:134-146, 297-316); image_config = the scan
 * of tsg_image_config_content's output (file "config.json"), or NULL, merged
 * as local/scan.go:487-496 does; then secretsToResults (local/scan.go:236-254),
 * the severity part of filterSecrets (result/filter.go:154-169) and
 * json.MarshalIndent(report, "", "  ") + "\n".  Go iterates the merged
 * secrets map in random order; this report lists them by FilePath.  Free
 * *out with tsg_free. */
int tsg_report_json(const tsg_result* const* layers, const tsg_layer* layer_refs, uint32_t nlayers,
                    const tsg_result* image_config, const tsg_report_opts* opts, char** out, size_t* len);
/* The image-config secret analyzer's input (imgconf/secret/secret.go:44):
 * json.MarshalIndent(v1.ConfigFile, "  ", "") of the config decoded from
 * config_json.  Scan it as ScanArgs{FilePath: "config.json"}.  Free with tsg_free. */
int tsg_image_config_content(const char* config_json, size_t config_len, char** out, size_t* len);
/* Base-layer secret skip (artifact/image/image.go:331-335, 526-554;
 * image/image.go:111-137): is_base[i] = 1 when layer diff_ids[i] belongs to
 * the base image, whose layers are analysed without the secret analyzer. */
int tsg_guess_base_layers(const char* config_json, size_t config_len, const char* const* diff_ids, uint32_t n,
                          uint8_t* is_base);

/* ---- client/server wire format ---- */
/* proto.Marshal of the trivy.common.Secret message (rpc/common/service.proto:
 * 152-156, 191-223) that ConvertToRPCSecrets (pkg/rpc/convert.go:146-175)
 * makes of file `file` of the result.  layers: NULL (every finding's Layer is
 * the empty message, as an fs scan) or one tsg_layer per finding.  Fails with
 * TSG_ERR_INVALID where proto.Marshal fails: a string that is not valid UTF-8.
 * Free *out with tsg_free. */
int tsg_result_to_proto(const tsg_result* r, size_t file, const tsg_layer* layers, char** out, size_t* len);
/* proto.Unmarshal of n Secret messages + ConvertFromRPCSecrets
 * (convert.go:504-533): a result with one types.Secret per message; the
 * findings' Layers appear in tsg_result_json as "Layer". */
int tsg_result_from_proto(const char* const* msgs, const size_t* lens, size_t n, tsg_result** out);

#ifdef __cplusplus
}
#endif

#endif /* TRIVY_SECRET_H_ */
