/*
 * trivy_secret_test.h -- test, measurement and tooling hooks of
 * libtrivysecret.so (the product C-ABI is trivy_secret.h).
 *
 * Nothing here has a reference analogue and no product entry point calls any
 * of it: CPU models of the GPU passes (for tests without a GPU), probes that
 * time one component, restated-Go-library probes checked against the
 * oracle, and fault injection for the per-file queue.
 */
#ifndef TRIVY_SECRET_TEST_H_
#define TRIVY_SECRET_TEST_H_

#include "trivy_secret.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Test hook: Go encoding/json string encoding of s (json.Marshal; with
 * escape_html = 0 as an Encoder with SetEscapeHTML(false)).  Free with tsg_free. */
int tsg_go_json_string(const uint8_t* s, size_t n, int escape_html, char** out, size_t* len);

/* Run only the two GPU passes; the result carries stats and candidates but no
 * findings (used to time the kernels in isolation). */
int tsg_prefilter_resident(tsg_engine* e, const void* d_data, const uint8_t* h_data,
                           const uint64_t* offsets, uint32_t nfiles, tsg_result** out);

/* Raw GPU candidates of file i for rule j (sorted starts); for tests.  Rule
 * indices past tsg_ruleset_num_rules are the exclude-block pseudo-rules, in
 * the order of the prefilter report. */
int tsg_result_candidates(const tsg_result* r, uint32_t file, uint32_t rule, const uint64_t** starts, size_t* n);
/* The (file, rule) pairs of r that have candidates, as 2 * *n uint32 in
 * ascending order (free with tsg_free): what to ask tsg_result_candidates
 * for.  Tests only; never used by tsg_scan_batch. */
int tsg_result_candidate_keys(const tsg_result* r, uint32_t** keys, size_t* n);
/* K1's other outputs as tsg_prefilter_resident read them back: the '\n' count
 * of every *chunk_bytes-byte chunk of the packed batch (*n = the number of
 * chunks; the pointers live as long as r), and one flag word per file.  Tests
 * only; never used by tsg_scan_batch. */
int tsg_result_chunk_newlines(const tsg_result* r, const uint16_t** counts, size_t* n, uint32_t* chunk_bytes);
int tsg_result_file_flags(const tsg_result* r, const uint32_t** flags, size_t* n);
/* Test hook: while `on`, the results of tsg_scan_batch and
 * tsg_scan_batch_resident on this engine carry, next to the findings, the raw
 * outputs of the GPU passes as Engine::scan saw them, segment by segment:
 *  - every real file's candidates, in batch file indices and file-relative
 *    starts, sorted and de-duplicated per (file, rule)
 *    (tsg_result_candidates, tsg_result_candidate_keys), and its flag word
 *    (tsg_result_file_flags, one per file of the batch);
 *  - one record per segment, in segment order (tsg_result_raw_segments,
 *    tsg_result_raw_segment): where the batch was cut, the segment's K1 chunk
 *    size, its '\n' count per chunk (the chunk grid starts at the lead, b0 -
 *    lead_bytes, when the segment has one), its K1 anchor hits (the lead's
 *    included), and what the passes said about the lead -- the pseudo-file of
 *    the bytes between the 256-byte boundary below a resident piece's first
 *    file and that file, whose results the product drops: its flag word, the
 *    number of candidates K2 emitted for it and their distinct (rule, start)
 *    pairs in ascending order.
 * The pointers of a record live as long as r.  Off (the default), a scan takes
 * one more branch per segment and copies nothing.  No product entry point
 * calls it. */
typedef struct {
  uint32_t f0, nfiles, lead;       /* first file of the batch; the segment's own files; 1 = it ran with a lead */
  uint32_t chunk_bytes;            /* K1 chunk bytes of this segment */
  uint64_t b0, bytes, lead_bytes;  /* first byte of f0 in the batch; bytes of the own files; bytes of the lead */
  uint64_t hits;                   /* K1 anchor hits, the lead's included */
  uint32_t lead_flags;             /* the lead's flag word */
  uint32_t lead_emitted;           /* candidates K2 emitted for the lead, duplicates included */
  const uint16_t* chunk_newlines;  /* nchunks counts */
  size_t nchunks;
  const uint32_t* lead_cand_rules; /* nlead_cands distinct (rule, start) pairs of the lead */
  const uint64_t* lead_cand_starts;
  size_t nlead_cands;
} tsg_raw_segment;
int tsg_test_keep_raw(tsg_engine* e, int on);
int tsg_result_raw_segments(const tsg_result* r, size_t* n);
int tsg_result_raw_segment(const tsg_result* r, size_t k, tsg_raw_segment* rec);

/* The device-only scan's gather layout (csrc/gather.h: plan_gather, the CPU
 * model of gather.hip's device scan) on an offsets array alone: files below
 * `lead` are never gathered, need[f] != 0 marks a file the confirmer reads,
 * chunk = the segment's K1 chunk bytes.  goff (nfiles uint64) receives each
 * file's first byte in the gather buffer or UINT64_MAX; runs (3 uint64 per
 * run: source in the segment's frame, destination, length; runs_cap runs)
 * the run table, *nruns its size (set even when it exceeds runs_cap, which
 * fails), *total the buffer bytes taken.  Tests only. */
int tsg_test_plan_gather(const uint64_t* offsets, uint32_t nfiles, uint32_t lead, const uint8_t* need, uint32_t chunk,
                         uint64_t* goff, uint64_t* runs, size_t runs_cap, size_t* nruns, uint64_t* total);
/* Test hook: while `on`, a tsg_scan_batch_device result keeps, per segment
 * (in segment order, as tsg_result_raw_segment, whose records it also keeps),
 * the gather as it came back from the device -- over the segment's files in
 * its own frame, the lead (if any) as file 0 and offsets counted from the
 * chunk grid's origin b0 - lead_bytes: need, goff, the run table, the buffer
 * bytes taken and those bytes; and the buffer's capacity at each
 * tsg_gather_copy launch with, per launch, whether the 4096-byte 0xA5 pattern
 * the hook writes past that capacity was still whole afterwards.  While on,
 * tsg_prefilter_resident called with h_data NULL runs the gather behind its
 * two passes as well and keeps the one segment's record (no confirmation:
 * for batches whose confirmation takes long).  Off by default.  No product
 * entry point calls it. */
typedef struct {
  uint32_t nfiles;                 /* the segment's files, the lead included */
  const uint8_t* need;
  const uint64_t* goff;
  const uint64_t* runs;            /* nruns x (source, destination, length) */
  size_t nruns;
  uint64_t total;                  /* gather_total */
  const uint64_t* caps;            /* ncaps capacities, one per copy launch that was waited for */
  const uint8_t* guard_ok;
  size_t ncaps;
  const uint8_t* bytes;            /* total bytes of the gather buffer */
} tsg_gather_segment;
int tsg_test_keep_gather(tsg_engine* e, int on);
int tsg_result_gather_segment(const tsg_result* r, size_t k, tsg_gather_segment* rec);
/* Test hook: gather buffers the engine's devices own, those back in their
 * pool (all of them between scans), and their bytes. */
int tsg_test_gather_pool(tsg_engine* e, uint32_t* buffers, uint32_t* idle, uint64_t* bytes);
/* CPU model of the device-only scan (tests without a GPU): the table model's
 * candidates and flags, plan_gather with K1 chunks of `chunk` bytes, the runs
 * copied into a buffer of exactly the gather's size, and the engine's
 * confirmation of a segment without a host copy reading that buffer.  The
 * result carries the findings, the gather stats and one gather record
 * (tsg_result_gather_segment 0).  Never used by a scan. */
int tsg_scan_device_model(const tsg_ruleset* rs, const uint8_t* data, const uint64_t* offsets, uint32_t nfiles,
                          const char* const* paths, const uint32_t* path_lens, const uint8_t* binary,
                          uint32_t chunk, tsg_result** out);
/* The same; release(user) (may be NULL) is called once the gather is made and
 * before the confirmation starts: `data` is not read after it, so the caller
 * may free the batch there -- under a host sanitizer a stray read through the
 * batch's old address then shows (tools/asan_driver.cpp --device-model). */
int tsg_scan_device_model_release(const tsg_ruleset* rs, const uint8_t* data, const uint64_t* offsets, uint32_t nfiles,
                                  const char* const* paths, const uint32_t* path_lens, const uint8_t* binary,
                                  uint32_t chunk, void (*release)(void* user), void* user, tsg_result** out);

/* The device-only scan with windows (tsg_scan_batch_device_opts), on the CPU.
 *
 * tsg_test_plan_gather_windows: csrc/gather.h plan_gather_windows, the CPU
 * model of gather.hip's window passes, on plain arrays -- the candidate list
 * as three parallel arrays (duplicates and any order allowed), the per-file
 * flag words, whether the rule set has a mode-1 rule, and the windowable byte
 * per row of the rule table.  cls (nfiles: 0 none, 1 whole, 2 windowed),
 * first_run (nfiles: the run holding the file's first chunk or UINT32_MAX),
 * marks (may be NULL; one byte per chunk of the segment), the run table as
 * tsg_test_plan_gather's.
 * tsg_test_windowable_rows: that byte table for a rule set (rules, then
 * exclude-block pseudo-rules).
 * tsg_test_regex_examined: the anchored run of `pattern` at text[pos] on the
 * text cut at len, by the capture path (submatch != 0) or the match-end path,
 * with the furthest byte index it asked for (len: the end of the text).
 * tsg_scan_device_model_opts: tsg_scan_device_model_release with windows --
 * the table model's candidates, plan_gather_windows, every run copied into an
 * allocation of exactly its bytes, the windowed confirmation, and the
 * fallback round (plan_gather over the insufficient files, a buffer of
 * exactly its size).  The result holds two gather records: 0 the windowed
 * round (tsg_result_window_segment 0 adds the classes and the insufficient
 * files), 1 the fallback's.  opts NULL or 0/0: tsg_scan_device_model_release.
 * A tsg_scan_batch_device_opts result made with tsg_test_keep_raw and
 * tsg_test_keep_gather on holds, when files fell back, one more record behind
 * its segments' (index tsg_result_raw_segments - 1): the fallback round's
 * gather over the batch's files -- need, goff into the round's one buffer, the
 * run table with sources in the batch's frame, the bytes, the buffer's
 * capacity and whether the guard pattern behind it was whole.
 *
 * With a line cap (tsg_device_scan_opts2.window_line_cap):
 * tsg_test_plan_gather_lines is tsg_test_plan_gather_windows with the frame's
 * bytes (data: offsets[nfiles] bytes; csrc/gather.h line_window walks them
 * directly, with no table) and the two line counters (may be NULL); it also
 * runs the device pass's walk (line_window_chunks, on the '\n' count per
 * chunk of `data`) and fails with TSG_ERR_INTERNAL when the two plans differ;
 * tsg_scan_device_model_opts2 is tsg_scan_device_model_opts with the cap,
 * fallback round included.  Cap 0 gives the plain functions' output. */
typedef struct {
  uint32_t nfiles;
  const uint8_t* cls;
  const uint32_t* insufficient;    /* ascending file indices of the segment */
  size_t ninsufficient;
} tsg_window_segment;
int tsg_test_plan_gather_windows(const uint64_t* offsets, uint32_t nfiles, uint32_t lead, const uint32_t* cand_files,
                                 const uint32_t* cand_rules, const uint64_t* cand_starts, size_t ncands,
                                 const uint32_t* fflags, int all, const uint8_t* windowable, uint32_t nrows,
                                 uint32_t chunk, const tsg_device_scan_opts* opts, uint8_t* cls, uint32_t* first_run,
                                 uint8_t* marks, uint64_t* runs, size_t runs_cap, size_t* nruns, uint64_t* total);
int tsg_test_windowable_rows(const tsg_ruleset* rs, uint8_t* rows, size_t cap, size_t* nrows, size_t* nrules);
int tsg_test_regex_examined(const char* pattern, const uint8_t* text, size_t len, size_t pos, int submatch, long* end,
                            size_t* examined);
int tsg_result_window_segment(const tsg_result* r, size_t k, tsg_window_segment* rec);
int tsg_scan_device_model_opts(const tsg_ruleset* rs, const uint8_t* data, const uint64_t* offsets, uint32_t nfiles,
                               const char* const* paths, const uint32_t* path_lens, const uint8_t* binary,
                               uint32_t chunk, const tsg_device_scan_opts* opts, void (*release)(void* user),
                               void* user, tsg_result** out);
int tsg_test_plan_gather_lines(const uint8_t* data, const uint64_t* offsets, uint32_t nfiles, uint32_t lead,
                               const uint32_t* cand_files, const uint32_t* cand_rules, const uint64_t* cand_starts,
                               size_t ncands, const uint32_t* fflags, int all, const uint8_t* windowable,
                               uint32_t nrows, uint32_t chunk, const tsg_device_scan_opts2* opts, uint8_t* cls,
                               uint32_t* first_run, uint8_t* marks, uint64_t* runs, size_t runs_cap, size_t* nruns,
                               uint64_t* total, uint64_t* widened, uint64_t* capped);
int tsg_scan_device_model_opts2(const tsg_ruleset* rs, const uint8_t* data, const uint64_t* offsets, uint32_t nfiles,
                                const char* const* paths, const uint32_t* path_lens, const uint8_t* binary,
                                uint32_t chunk, const tsg_device_scan_opts2* opts, void (*release)(void* user),
                                void* user, tsg_result** out);

/* CPU model of tsg_prepare_batch_device (csrc/prep.h: plan_prep, the device
 * pass stated sequentially with its per-byte rule: a byte of a binary .pyc is
 * kept iff it is printable and lies in a window of 5 printable bytes of its
 * file, and a '\n' follows a kept byte whose successor is not printable or is
 * the file's end) behind the same host gate.  *out is an ordinary
 * tsg_prepared with the bytes on the host; kinds (nfiles bytes, may be NULL)
 * receives 0 dropped / 1 text / 2 printable runs per raw file, new_offsets
 * (nfiles + 1, may be NULL) every raw file's start in the prepared bytes.
 * Tests only; the independent restatement it is checked against is
 * tsg_prepare_batch_opts. */
int tsg_prepare_device_model(const tsg_ruleset* rs, const uint8_t* raw, const uint64_t* raw_offsets, uint32_t nfiles,
                             const char* const* paths, const uint32_t* path_lens, const tsg_feed_opts* opts,
                             uint8_t* kinds, uint64_t* new_offsets, tsg_prepared** out);
/* The device pass's printable table (re::is_print of the 256 byte values) as
 * 256 bytes of 0 / 1.  Tests only. */
int tsg_prepare_print_table(uint8_t* table);
/* Measurement hook: the kernel times (ms) of the four passes of the
 * tsg_prepare_batch_device call that made p -- classify, count, scan,
 * compact (tools/prep_probe.py). */
int tsg_prepared_pass_ms(const tsg_prepared* p, double* pass_ms);

/* What the device walk of tsg_prepare_layer_tar_device marks (csrc/tarscan.h
 * plan_tar_marks, the CPU statement of tarscan.hip): marks[b] = 1, b < len /
 * 512, for every whole block that passes the header checksum test and for the
 * payload blocks behind an 'x' / 'g' / 'L' / 'K' header with 0 <= size <= 1
 * MiB, else 0.  Tests only. */
int tsg_test_tar_marks(const uint8_t* tar, uint64_t len, uint8_t* marks);
/* csrc/tarscan.h tar_block_is_header of n 512-byte blocks (is[k] = 0 / 1).  Tests only. */
int tsg_test_tar_is_header(const uint8_t* blocks, uint64_t n, uint8_t* is);
/* The device's mark / compact pass alone over d_tar[0, len) (16-byte aligned
 * device memory): *n = marked blocks; when *n <= cap, idx[0..*n) their block
 * numbers in order and blocks_out their 512 * *n bytes.  Tests only. */
int tsg_test_tar_scan_device(tsg_engine* e, const void* d_tar, uint64_t len, uint64_t* idx, uint64_t cap, uint64_t* n,
                             uint8_t* blocks_out);
/* CPU model of tsg_prepare_layer_tar_device (tests without a GPU): marks ->
 * SparseTarInput over a host copy -> walk_layer -> gate -> interleaved
 * entries -> plan_prep.  use_marks = 0: nothing is gathered, every read of
 * the walk is a fallback.  *fallback_reads (may be NULL) = reads not served
 * by the marked blocks, also when the walk fails; *out: an ordinary
 * tsg_prepared with the bytes on the host, paths and walk JSON as the device
 * call's.  The independent restatement it is checked against is
 * tsg_prepare_layer_tar_opts. */
int tsg_prepare_layer_tar_device_model(const tsg_ruleset* rs, const uint8_t* tar, uint64_t len,
                                       const tsg_feed_opts* opts, int use_marks, uint32_t* fallback_reads,
                                       tsg_prepared** out);

/* Bit of a file's flag word (engine.h kFileFoldSpecial): the file holds
 * U+0130, U+212A or U+017F, so the host scans it with the variant tables.  K1
 * may also set it for a file that shares a 16-byte word of the batch with such
 * a sequence of a neighbouring file (a superset is safe). */
#define TSG_FILE_FOLD_SPECIAL 1u

/* CPU model of K1 + K2 alone: prefilter_reference_file on every file -- the
 * base tables the engine runs (K1c's compressed table when the rule set has
 * one), no variant pass for fold-special files, no confirmer.  The result
 * carries the candidates (tsg_result_candidates), one flag word per file
 * (tsg_result_file_flags: TSG_FILE_FOLD_SPECIAL where the model says
 * fold-special) and, in its stats, the anchor hits and the distinct
 * candidates.  The GPU passes must produce exactly these sets
 * (tests/test_gpu_candidates.py).  Never used by tsg_scan_batch. */
int tsg_prefilter_table_model(const tsg_ruleset* rs, const uint8_t* data, const uint64_t* offsets, uint32_t nfiles,
                              tsg_result** out);

/* Host exact confirmer evaluated on every (file, rule) pair with no GPU
 * prefilter (the reference algorithm restated in C++).  For tests of the
 * confirmer; never used by tsg_scan_batch. */
int tsg_scan_host_reference(const tsg_ruleset* rs, const uint8_t* data, const uint64_t* offsets,
                            uint32_t nfiles, const char* const* paths, const uint32_t* path_lens,
                            const uint8_t* binary, int threads, tsg_result** out);
/* CPU model of the GPU tables (K1+K2 semantics) feeding the confirmer; for
 * tests of the compiled prefilter without a GPU.  Never used by tsg_scan_batch. */
int tsg_scan_table_model(const tsg_ruleset* rs, const uint8_t* data, const uint64_t* offsets,
                         uint32_t nfiles, const char* const* paths, const uint32_t* path_lens,
                         const uint8_t* binary, tsg_result** out);
/* Prefilter compile report without a GPU (NUL-terminated; free with tsg_free). */
int tsg_prefilter_report(const tsg_ruleset* rs, char** out);
/* Tooling (no reference analogue): scan DFA `group` as compiled for K1 --
 * next[state * nclasses + class] (state ids), byte -> class map (256 bytes),
 * states >= first_out have outputs.  Both arrays are freed with tsg_free. */
int tsg_scan_dfa_dump(const tsg_ruleset* rs, uint32_t group, uint16_t** next, uint8_t** byte_class,
                      uint32_t* nstates, uint32_t* nclasses, uint32_t* first_out);
/* Test hook for the host regexp engine: compiles `pattern` (Go syntax) and,
 * for each of the n positions, writes the end of the leftmost-first match
 * anchored there (-1: none) as computed by the lazy DFA (dfa_end) and by
 * match_at's anchored path (vm_end: the bit-state backtracker where Go would
 * use it, else the Pike VM); fails with TSG_ERR_INTERNAL if the scanner's own
 * match_end (span shape / backtracker / lazy DFA) differs from vm_end.  Never
 * used by tsg_scan_batch. */
int tsg_regex_probe(const char* pattern, const uint8_t* text, size_t len, const uint64_t* pos, size_t n,
                    int64_t* dfa_end, int64_t* vm_end);
/* Test hook for the Go sort.Slice restatement (gosort.h, pdqsort_func of
 * go1.23 sort/zsortfunc.go as scanner.go:452-457 uses it): order[] = 0..n-1
 * sorted by keys[order[i]] < keys[order[j]] -- unstable, so ties keep Go's
 * order only if the algorithm is Go's.  Never used by tsg_scan_batch. */
int tsg_test_go_sort(const uint32_t* keys, size_t n, uint32_t* order);
/* Test hook for the engine's readback kernel (tsg_readback, engine.hip) on
 * HIP device 0: copies min(nwords, count * per_count) dwords (the product in
 * 64 bits) of a device buffer filled with 1, 2, ... into host-mapped memory;
 * *copied = the dwords that arrived.  Never used by tsg_scan_batch. */
int tsg_test_readback(uint32_t nwords, uint32_t count, uint32_t per_count, uint32_t* copied);

/* Test hook: the engine's host footprint so far -- lanes (a compute and a
 * copy stream plus device scratch each) created over all its devices, call
 * contexts, and confirm-pool threads started.  Never used by tsg_scan_batch. */
int tsg_test_engine_footprint(tsg_engine* e, uint32_t* lanes, uint32_t* calls, uint32_t* pool_threads);

/* CPU model of the engine's multi-device segment pipeline (pipeline.h:
 * DriverPipeline, the code Engine::scan runs its device drivers on) with
 * simulated devices: `ndevices` drivers, each holding a lane of its device's
 * pool, pull `nsegments` segments (seg_us of "GPU" work each) and hand them to
 * the calling thread, which confirms each (confirm_us).  fail_mode 1: driver
 * fail_device returns an error at its fail_at-th segment (a HIP error); 2: it
 * throws bad_alloc there; 3: the confirming thread throws at its fail_at-th
 * segment; 0: no failure.  Returns TSG_OK, or the failure's code and message;
 * *out tells what ran.  Tests only (tests/test_pipeline_model.py). */
typedef struct {
  uint64_t segments_started, segments_pushed, segments_confirmed, segments_confirmed_twice;
  uint64_t started_after_failure;  /* segments any driver began after the failure */
  uint32_t lanes_outstanding;      /* lanes not back in their pools when the call returned */
  uint32_t lanes_created;          /* most lanes a pool had out at once, summed over devices */
  uint32_t drivers_alive;          /* driver bodies still running when the call returned */
  double wall_ms, fail_to_return_ms;
} tsg_model_pipeline_stats;
int tsg_test_multi_driver_model(uint32_t ndevices, uint32_t nsegments, int32_t fail_device, uint32_t fail_at,
                                uint32_t fail_mode, uint32_t seg_us, uint32_t confirm_us,
                                tsg_model_pipeline_stats* out);

/* The engine's segment planner (csrc/segments.h: plan_segments, the code
 * Engine::scan cuts a batch with) on an offsets array alone: no engine, no
 * device.  resident: the batch is device-resident at address `base` (used only
 * for the 256-byte alignment of the pieces); with_paths 0: the batch has no
 * paths (no lead files, as in the engine).  out[0, *nout) describes the
 * segments (*nout is set even when it exceeds out_cap, which fails); rebased
 * (may be NULL) receives each segment's nfiles + 1 rebased offsets, one
 * segment after the other.  Tests only (tests/test_segments.py). */
typedef struct {
  uint32_t pieces;                 /* TSG_PIECES */
  double first_piece, first_piece_few, last_piece;
  uint64_t min_piece, segment, segment_min;
  int32_t balanced;
  double dense_files_per_gb;       /* the engine's kDenseFilesPerGB: 8000 */
} tsg_segment_policy;
typedef struct {
  uint32_t f0, nfiles, lead;       /* first file of the batch; files with the lead; 1 = file 0 is a lead */
  uint64_t b0, bytes;              /* first byte of f0 in the batch; bytes of the segment's own files */
  uint64_t d_data;                 /* resident: the segment's device address (the lead's, if any) */
} tsg_segment_info;
int tsg_test_plan_segments(const uint64_t* offsets, uint32_t nfiles, int resident, uint64_t base, int with_paths,
                           const tsg_segment_policy* pol, tsg_segment_info* out, uint32_t out_cap, uint32_t* nout,
                           uint64_t* rebased, size_t rebased_cap);

/* The wire feeder's strip planner (csrc/wire_strips.h: plan_wire_strips, the
 * code WireFeed cuts a segment into packer / copy strips with) on sizes alone:
 * offsets[i], bytes[i] of strip i, i < *nout (*nout is set even when it
 * exceeds cap, which fails).  first_segment 1: the scan's first segment, which
 * gets the ramp of small strips where the rules allow one.  Tests only
 * (tests/test_wire_strips.py). */
int tsg_test_plan_wire_strips(uint64_t segment_bytes, uint64_t strip, int first_segment, int npackers,
                              uint64_t* offsets, uint64_t* bytes, uint32_t cap, uint32_t* nout);

/* K1's work-item schedule as the host restates it (csrc/k1_schedule.h; the
 * kernel, tsg_k1_scan_v3, keeps its own arithmetic) for a launch of nchunks
 * chunks on a grid of `blocks` workgroups of 16 waves with `rounds` tail
 * rounds (TSG_K1_TAIL_ROUNDS) and, top8 != 0, the 8-chunk bulk level: no
 * engine, no device.  levels[0..5] = the chunks of the 8-, 4-, 2- and 1-chunk
 * levels (in batch order), the number of wave items, and k1_grid_ok (1: every
 * item has a taker -- the check Engine::seg_prologue fails a segment on).
 * items (may be NULL; 3 uint64 per item, items_cap items, which must hold
 * them all) receives each item's kU, first chunk c0 and level end rend: lane
 * j walks the chunks [c0 + j * kU, min(c0 + (j + 1) * kU, rend)).  Tests only
 * (tests/test_schedule_corpus.py). */
int tsg_test_k1_schedule(uint64_t nchunks, uint32_t blocks, uint32_t rounds, int top8, uint64_t* levels,
                         uint64_t* items, size_t items_cap);

/* Test hook: the engine's next n segment runs fail before their first
 * launch (as a failed device allocation would), so a test can check that a
 * failed call leaves nothing behind on the engine's pooled lanes.  Never used
 * by tsg_scan_batch. */
int tsg_test_inject_segment_failures(tsg_engine* e, uint32_t n);

/* Test hook for the wire packing (csrc/wirepack.h): packs src[0, n) as one
 * strip on the host -- path 0: the CPU's best, 1: scalar, 2: AVX2 (scalar on a
 * CPU without it; *path_used tells which ran) -- into packed (packed_cap
 * bytes; n + 8 always suffices) and table (one entry per 4096-byte block:
 * offset in packed, bit 31 set for a block sent unchanged); *packed_len = the
 * packed bytes.  back (n bytes, may be NULL) receives the host unpack of the
 * result.  Never used by tsg_scan_batch. */
int tsg_test_wire_pack(const uint8_t* src, size_t n, int path, uint8_t* packed, size_t packed_cap, uint32_t* table,
                       size_t* packed_len, int* path_used, uint8_t* back);
/* Test hook: uploads a packed strip to HIP device 0, runs the unpack kernel
 * and reads the n restored bytes back into out; fails if the kernel wrote
 * past them.  Never used by tsg_scan_batch. */
int tsg_test_wire_unpack_device(const uint8_t* packed, size_t packed_len, const uint32_t* table, size_t n,
                                uint8_t* out);
/* The same two hooks for the 6-bit codec with escapes (csrc/wirepack.h, "v2").
 * path 0: the CPU's best, 1: scalar, 2: AVX2, 3: AVX-512 VBMI (the best path
 * below it on a CPU without the one asked for; *path_used tells which ran).
 * packed: n + 16 bytes always suffice.  table: one entry per block, bit 31 set
 * for a raw block, bit 30 for a 6-bit one.  alpha: the strip's alphabets, 64
 * bytes per 64 KiB region rounded up to a multiple of 256 bytes in all.
 * counts (4 values, may be NULL): 6-bit, 7-bit and raw blocks, escaped bytes. */
int tsg_test_wire_pack2(const uint8_t* src, size_t n, int path, uint8_t* packed, size_t packed_cap, uint32_t* table,
                        uint8_t* alpha, size_t* packed_len, int* path_used, uint64_t* counts, uint8_t* back);
int tsg_test_wire_unpack2_device(const uint8_t* packed, size_t packed_len, const uint32_t* table, const uint8_t* alpha,
                                 size_t n, uint8_t* out);
/* tsg_test_wire_pack2 with split blocks allowed (a table entry with bits 31
 * and 30 both set).  *vbmi2 (may be NULL): whether path 3 packs them with
 * AVX-512 VBMI2 on this CPU.  counts: 5 values, the fifth the split blocks;
 * the escaped bytes count those of 6-bit and split blocks.  The device hook
 * is the v2 one under the format's other name. */
int tsg_test_wire_pack3(const uint8_t* src, size_t n, int path, uint8_t* packed, size_t packed_cap, uint32_t* table,
                        uint8_t* alpha, size_t* packed_len, int* path_used, int* vbmi2, uint64_t* counts, uint8_t* back);
int tsg_test_wire_unpack3_device(const uint8_t* packed, size_t packed_len, const uint32_t* table, const uint8_t* alpha,
                                 size_t n, uint8_t* out);

/* The same two pipelines with the CPU model of the GPU passes as the scan
 * stage (tsg_scan_table_model's); tests only, never the product path. */
int tsg_scan_layer_stream_model(const tsg_ruleset* rs, tsg_read_fn read, void* user, const tsg_feed_opts* opts,
                                uint64_t batch_bytes, tsg_result** out);
int tsg_scan_fs_tree_model(const tsg_ruleset* rs, const char* root, const tsg_feed_opts* opts, uint64_t batch_bytes,
                           tsg_result** out);

/* Measurement hook: `callers` threads, each calling tsg_queue_scan on the
 * next not yet scanned file of the batch until all nfiles are done (the
 * reference's goroutines calling Scan per file); *seconds = wall time,
 * *findings = findings over all files.  Never used by tsg_scan_batch. */
int tsg_queue_probe(tsg_queue* q, const uint8_t* data, const uint64_t* offsets, uint32_t nfiles,
                    const char* const* paths, const uint32_t* path_lens, uint32_t callers, double* seconds,
                    uint64_t* findings);

/* Test hook: Regexp.MatchString(text) for `pattern` with the required-literal
 * gate the ruleset compiler sets on path / allow regexes (*gated) and without
 * it (*plain); *has_gate = 1 if a gate was found (2: bounded). */
int tsg_regex_match_probe(const char* pattern, const uint8_t* text, size_t len, int* gated, int* plain,
                          int* has_gate);

/* Test hook: a result holding the JSON array of types.Secret given (Go field
 * names), to check report assembly against the reference's types.Secret
 * fixtures.  Never used by a scan. */
int tsg_result_from_json(const char* json, size_t len, tsg_result** out);
/* Test hook: time.Time JSON round trip (RFC 3339 in, MarshalJSON's form out). */
int tsg_go_time_rfc3339(const char* in, char* out, size_t cap);

/* The per-file queue (tsg_queue_*) with the CPU model of the GPU passes as its
 * batch stage (tsg_scan_table_model's), for tests without a GPU.  fail_path
 * (may be NULL): a batch holding a file with this path throws std::bad_alloc
 * inside the stage, as an allocation failure inside the engine would; every
 * caller in that batch gets the error, the queue goes on.  Destroy with
 * tsg_queue_destroy. */
int tsg_queue_create_model(const tsg_ruleset* rs, uint32_t max_files, uint64_t max_bytes, uint32_t max_wait_us,
                           uint32_t max_inflight, const char* fail_path, tsg_queue** out);
/* Leaders of the queue that waited the full max_wait_us for callers that did
 * not come. */
int tsg_queue_timeouts(tsg_queue* q, uint64_t* timeouts);

/* The CPU model of tsg_inflate_gzip_device (inflate.h's inflate_model): the
 * same arguments with gz and dst in host memory and e unused (may be NULL);
 * status[] and out_lens[] are what the device call gives.  Nothing outside a
 * stream's slot is written. */
int tsg_test_inflate_model(tsg_engine* e, const void* gz, const uint64_t* gz_offsets, uint32_t nstreams, void* dst,
                           const uint64_t* dst_offsets, uint64_t* out_lens, int32_t* status, double* ms);
/* The checksum pass on the CPU: the CRC32 of data[0, len) taken in slices of
 * *slice bytes (crc32_slices) and folded with the shift operator
 * (crc32_combine); *nslices = the slices taken.  Any out pointer may be NULL. */
int tsg_test_crc32_slices(const uint8_t* data, uint64_t len, uint32_t* crc, uint32_t* slice, uint64_t* nslices);
/* The kernel times of the calling thread's last tsg_inflate_gzip_device call
 * (tools/inflate_probe.py): the inflate and the checksum kernel in ms, the
 * members it found and the slices it summed.  Any pointer may be NULL. */
int tsg_test_inflate_last_stats(double* inflate_ms, double* crc_ms, uint64_t* members, uint64_t* slices);

/* The CPU model of tsg_inflate_zstd_device (zstdec.h's zstd_model): the same
 * arguments with z and dst in host memory and e unused (may be NULL);
 * status[] and out_lens[] are what the device call gives.  Nothing outside a
 * stream's slot is written. */
int tsg_test_zstd_model(tsg_engine* e, const void* z, const uint64_t* z_offsets, uint32_t nstreams, void* dst,
                        const uint64_t* dst_offsets, uint64_t* out_lens, int32_t* status, double* ms);
/* What one stream exercises, counted by the model while it decodes it into a
 * slot of cap bytes of its own: counters[0, ncounters) in the order of
 * zstdec.h's kEv* (tools/gen_zstd_corpus.py holds the names); *status = the
 * stream's status. */
int tsg_test_zstd_trace(const uint8_t* z, size_t len, uint64_t cap, uint64_t* counters, uint32_t ncounters, int32_t* status);
/* The kernel times of the calling thread's last tsg_inflate_zstd_device call
 * (tools/zstd_probe.py): the decode and the hash kernel in ms, the frames and
 * blocks it decoded.  Any pointer may be NULL. */
int tsg_test_zstd_last_stats(double* decode_ms, double* hash_ms, uint64_t* frames, uint64_t* blocks);
/* XXH64 (seed 0) of data[0, len) as the checksum pass computes it */
int tsg_test_xxh64(const uint8_t* data, uint64_t len, uint64_t* hash);

#ifdef __cplusplus
}
#endif

#endif /* TRIVY_SECRET_TEST_H_ */
