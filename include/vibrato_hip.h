/*
 * vibrato_hip.h -- C ABI of libvibrato_hip.so: an MI355X (gfx950) drop-in for the
 * tokenize() hot path of daac-tools/vibrato 0.5.2.
 *
 * The reference has no FFI layer; its boundary is the public Rust API of crate
 * `vibrato` (vibrato/src/lib.rs:52-78).  Each entry point below names the Rust item
 * it replaces (paths relative to /root/reference/vibrato/src).  INTEGRATION.md shows
 * the Rust shim (`extern "C"` block + safe wrappers) a maintainer would add.
 *
 * Conventions
 *   - every fallible call returns a vbt_status; vbt_last_error() returns the
 *     thread-local message of the last failure (mirrors VibratoError, errors.rs:7-42)
 *   - handles are opaque; strings are {ptr,len} UTF-8, never NUL-terminated
 *   - tokenization never silently falls back to a CPU path: without a usable
 *     gfx950 device every vbt_tokenizer_* / vbt_*tokenize* call fails with VBT_ERR_DEVICE
 */
#ifndef VIBRATO_HIP_H
#define VIBRATO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VBT_API __attribute__((visibility("default")))

typedef enum vbt_status {
    VBT_OK = 0,
    VBT_ERR_INVALID_ARGUMENT = 1, /* VibratoError::InvalidArgument, errors.rs:13 */
    VBT_ERR_INVALID_FORMAT = 2,   /* VibratoError::InvalidFormat,   errors.rs:16 */
    VBT_ERR_INVALID_STATE = 3,    /* VibratoError::InvalidState,    errors.rs:19 */
    VBT_ERR_PARSE_INT = 4,        /* VibratoError::ParseInt,        errors.rs:25 */
    VBT_ERR_UTF8 = 5,             /* VibratoError::Utf8,            errors.rs:37 */
    VBT_ERR_DEVICE = 100,         /* HIP runtime / no gfx950 device (new: the reference is CPU-only) */
    VBT_ERR_UNSUPPORTED = 101     /* input outside what the device image can represent */
} vbt_status;

/* LexType, dictionary.rs:30-40 */
typedef enum vbt_lex_type { VBT_LEX_SYSTEM = 0, VBT_LEX_USER = 1, VBT_LEX_UNKNOWN = 2 } vbt_lex_type;

/* Output modes of the `tokenize` CLI, tokenize/src/main.rs:83-127 */
typedef enum vbt_format_mode { VBT_FORMAT_MECAB = 0, VBT_FORMAT_WAKATI = 1, VBT_FORMAT_DETAIL = 2 } vbt_format_mode;

typedef struct vbt_dict vbt_dict;
typedef struct vbt_tokenizer vbt_tokenizer;
typedef struct vbt_worker vbt_worker;
typedef struct vbt_batch vbt_batch;
typedef struct vbt_workspace vbt_workspace;

/* Fixed 24-byte token record written by the device (one per best-path node).
 * Fields are what Token::{range_char, range_byte, word_idx, total_cost} return
 * (token.rs:21-92); positions are relative to the sentence. */
typedef struct vbt_token_rec {
    uint32_t start_char, end_char; /* Token::range_char, token.rs:21-24 */
    uint32_t start_byte, end_byte; /* Token::range_byte, token.rs:28-32 */
    uint32_t word_idx;             /* WordIdx: lex_type << 30 | word_id (word_idx.rs:5-11) */
    int32_t total_cost;            /* Token::total_cost, token.rs:89-92 */
} vbt_token_rec;

/* Full token view (Token accessors, token.rs:21-92). surface points into the
 * caller's sentence bytes / batch copy, feature into dictionary memory. */
typedef struct vbt_token {
    const char* surface; size_t surface_len; /* Token::surface, token.rs:36-39 */
    const char* feature; size_t feature_len; /* Token::feature, token.rs:49-54 */
    uint32_t start_char, end_char, start_byte, end_byte;
    uint32_t lex_type, word_id;              /* Token::lex_type / word_idx */
    uint16_t left_id, right_id;              /* Token::left_id / right_id, token.rs:64-75 */
    int16_t word_cost;                       /* Token::word_cost, token.rs:78-87 */
    int32_t total_cost;
} vbt_token;

VBT_API const char* vbt_last_error(void);
/* 1 when the bytes are a Rust `str` (strict UTF-8), else 0: what every text-taking entry point requires. */
VBT_API int vbt_utf8_valid(const char* utf8, size_t len);

/* ---- Dictionary ------------------------------------------------------------ */

/* SystemDictionaryBuilder::from_readers(lex.csv, matrix.def, char.def, unk.def), builder.rs:64-89 */
VBT_API int vbt_dict_from_sources(const char* lex, size_t lex_len, const char* matrix_def, size_t matrix_len,
                                  const char* char_def, size_t char_len, const char* unk_def, size_t unk_len,
                                  vbt_dict** out);
/* Same, with the connection matrix given in binary: data[left*num_right+right] (the layout of
 * MatrixConnector, connector/matrix_connector.rs:11-15,47). A 459 MiB matrix has no sane text form. */
VBT_API int vbt_dict_from_sources_binmatrix(const char* lex, size_t lex_len, const int16_t* matrix,
                                            uint32_t num_right, uint32_t num_left, const char* char_def,
                                            size_t char_len, const char* unk_def, size_t unk_len, vbt_dict** out);
/* SystemDictionaryBuilder::from_readers_with_bigram_info(lex.csv, bigram.right, bigram.left, bigram.cost, char.def, unk.def,
 * dual_connector), builder.rs:111-160: the connection costs come from the compact bigram model (RawConnector
 * connector/raw_connector.rs; dual != 0: DualConnector connector/dual_connector.rs, a small matrix over classes of connection
 * ids + an 8-wide raw part, built as the reference builds it except that ties of its greedy template choice -- which the
 * reference resolves by hash-set iteration order -- go to the highest template index).  The device image materialises either as
 * a dense matrix when the tokenizer is created: i16 cells when every cost fits, else i32 cells (the reference's Raw / Dual cost is
 * an i32 sum, raw_connector.rs:153-161, dual_connector.rs:267-279); VBT_ERR_UNSUPPORTED there only for a matrix of 4 GiB or more. */
VBT_API int vbt_dict_from_sources_bigram(const char* lex, size_t lex_len, const char* bigram_right, size_t right_len,
                                         const char* bigram_left, size_t left_len, const char* bigram_cost, size_t cost_len,
                                         const char* char_def, size_t char_len, const char* unk_def, size_t unk_len, int dual,
                                         vbt_dict** out);
/* Dictionary::read(rdr), dictionary.rs:173-197: a dictionary written by Dictionary::write ("VibratoTokenizer 0.5\n" + bincode,
 * common.rs:5-9).  A zstd frame around it -- the released `system.dic.zst`, which the reference's CLIs unwrap with
 * zstd::Decoder (tokenize/src/main.rs:59-60) -- is detected by its magic and decompressed first (libzstd.so.1 of the system).
 * VBT_ERR_INVALID_ARGUMENT: wrong magic (dictionary.rs:188-193); VBT_ERR_INVALID_FORMAT: anything that does not decode. */
VBT_API int vbt_dict_read(const uint8_t* data, size_t len, vbt_dict** out);
/* Dictionary::write(wtr), dictionary.rs:142-150.  zstd_level < 0: the plain `system.dic` bytes; otherwise wrapped in a zstd
 * frame of that level like compile/src/main.rs:98 (level 19 there).  *out is released with vbt_free. */
VBT_API int vbt_dict_write(const vbt_dict* dict, int zstd_level, uint8_t** out, size_t* len);
/* ConnectorWrapper variant, connector.rs:30-35: 0 Matrix, 1 Raw, 2 Dual (-1: null / consumed handle) */
VBT_API int vbt_dict_connector_kind(const vbt_dict* dict);
/* Dictionary::reset_user_lexicon_from_reader(Some(csv) | None), dictionary.rs:209-229 */
VBT_API int vbt_dict_set_user_lexicon(vbt_dict* dict, const char* csv, size_t len);
/* Dictionary::map_connection_ids_from_iter(lmap, rmap), dictionary.rs:245-259: the i-th item (1-origin) is the
 * old id mapped to new id i; id 0 (BOS/EOS) is fixed. Permutes lexicon params, unknown entries and the matrix. */
VBT_API int vbt_dict_map_connection_ids(vbt_dict* dict, const uint16_t* lmap, size_t n_lmap, const uint16_t* rmap, size_t n_rmap);
VBT_API void vbt_dict_free(vbt_dict* dict);

VBT_API uint32_t vbt_dict_num_words(const vbt_dict* dict, uint32_t lex_type);
VBT_API uint32_t vbt_dict_num_left(const vbt_dict* dict);  /* Connector::num_left,  connector.rs:14 */
VBT_API uint32_t vbt_dict_num_right(const vbt_dict* dict); /* Connector::num_right, connector.rs:17 */
/* Dictionary::word_feature, dictionary.rs:108-114 */
VBT_API int vbt_dict_word_feature(const vbt_dict* dict, uint32_t lex_type, uint32_t word_id, const char** ptr, size_t* len);
/* Dictionary::word_param, dictionary.rs:98-104: out = {left_id, right_id, word_cost} */
VBT_API int vbt_dict_word_param(const vbt_dict* dict, uint32_t lex_type, uint32_t word_id, int32_t out[3]);
/* ConnectorCost::cost(right_id, left_id), connector.rs:25-28 */
VBT_API int vbt_dict_conn_cost(const vbt_dict* dict, uint32_t right_id, uint32_t left_id, int32_t* out);
/* CharProperty::char_info, character.rs:112-116 (packed CharInfo u32, character.rs:10-24) */
VBT_API uint32_t vbt_dict_char_info(const vbt_dict* dict, uint32_t code_point);
/* CharProperty::cate_id, character.rs:119-124; -1 when undefined */
VBT_API int vbt_dict_cate_id(const vbt_dict* dict, const char* name, size_t len);
/* Lexicon::common_prefix_iterator, lexicon.rs:33-46 (host walk of the device trie image).
 * out rows = {word_id, end_char}; returns the number of matches (may exceed cap). */
VBT_API uint32_t vbt_dict_common_prefix(const vbt_dict* dict, uint32_t lex_type, const uint32_t* code_points,
                                        uint32_t n, uint32_t* out, uint32_t cap);

/* ---- Tokenizer ------------------------------------------------------------- */

/* Tokenizer::new(dict).ignore_space(b)?.max_grouping_len(n), tokenizer.rs:26-74.
 * Consumes `dict` on success (Tokenizer::new moves it). Uploads the device image to
 * HIP device `device` (-1 = current device). max_grouping_len 0 = unlimited. */
VBT_API int vbt_tokenizer_new(vbt_dict* dict, int ignore_space, uint32_t max_grouping_len, int device,
                              vbt_tokenizer** out);
/* The same over several GPUs of the node (new; SURVEY.md 8(b) `device_mask`, as an explicit list): one replica of the device
 * image per listed HIP device.  The reference leaves parallelism to the caller -- one Worker per thread over a shared &Tokenizer
 * (worker.rs:9-19, tokenizer.rs:82-84); here one tokenizer spans the devices and vbt_tokenize_batch splits every batch into
 * `n_devices` contiguous shards balanced by bytes, runs them side by side (a pooled workspace + stream per device) and has every
 * device's DMA engines write its shard of the results into the ONE pinned result block at the shard's offset: a gather to the
 * caller, no collective.  Results are identical to a single-device tokenizer's.  A device may be listed more than once (two
 * shards in flight on one GPU; how the path is tested on a one-GPU box).  Worker and the vbt_workspace_* device API use the
 * first listed device. */
VBT_API int vbt_tokenizer_new_multi(vbt_dict* dict, int ignore_space, uint32_t max_grouping_len, const int* devices,
                                    uint32_t n_devices, vbt_tokenizer** out);
VBT_API uint32_t vbt_tokenizer_num_devices(const vbt_tokenizer* tok);
/* Connection-id locality, built in (the reference's `reorder` + `map` workflow -- map/src/reorder.rs:34-63,
 * MatrixConnector::map_connection_ids matrix_connector.rs:99-116, Dictionary::map_connection_ids_from_iter dictionary.rs:245-259,
 * docs/map.md -- without a caller action): the first batch of at least VBT_CONNID_MIN_SENTENCES (2048) sentences a tokenizer sees
 * has up to VBT_CONNID_SAMPLE (16384) of its sentences, spread evenly over the batch, copied aside by two small kernels on the call's
 * stream -- the call itself stays asynchronous: nothing is allocated, synchronised or waited for on the caller's side -- and a
 * background thread sweeps that sample once more with the connection-id counters on, sorts the ids by count and publishes a device
 * image whose matrix rows / columns and entry id pairs are renumbered hot ids first; launches enqueued from then on read it.
 * Results are bit-identical (a pure permutation) and nothing visible is in device ids: Token::left_id / right_id, vbt_dict_conn_cost,
 * vbt_dict_write, the connection-id counters (vbt_workspace_connid_counts, vbt_worker_*connid*) all stay in the dictionary's
 * numbering, and a mapping applied with vbt_dict_map_connection_ids before the tokenizer was created is kept underneath.
 * VBT_CONNID_REORDER=0 turns it off.  out[8] = {epoch of the image in use (0 = the dictionary's numbering, 1 = renumbered),
 * state (0 waiting for a large batch, 1 running, 2 done, 3 off), sentences sampled, the minimum batch size, microseconds the
 * calibration took, left ids moved, right ids moved, 0}; of the tokenizer's first device. */
VBT_API int vbt_tokenizer_connid_reorder_info(const vbt_tokenizer* tok, uint64_t out[8]);
/* The same calibration up front and synchronously, from host text (`n` sentences, `offsets[n + 1]`; at most VBT_CONNID_SAMPLE of them,
 * spread evenly, are used), on every device of the tokenizer: for callers who do not want the image to change under their first
 * batches (map/src/reorder.rs:34-63 run as a step of its own).  A no-op once a calibration has happened or when it is switched off. */
VBT_API int vbt_tokenizer_calibrate(const vbt_tokenizer* tok, const uint8_t* text, const uint64_t* offsets, uint64_t n);
/* Returns once no calibration is running on any device of the tokenizer, or after timeout_ms (< 0: no limit); *idle = 1 when none
 * is running.  (Benchmarks wait here behind their warm-up so that the counting sweep does not share the GPU with the timed region.) */
VBT_API int vbt_tokenizer_connid_reorder_wait(const vbt_tokenizer* tok, int64_t timeout_ms, int* idle);
/* Lattice density of the text the tokenizer has been seeing: candidates (lattice nodes before the sweep) per input byte of the last batch
 * that reported, on the tokenizer's first device; 0 = no batch yet.  ~2.0 on running Japanese text over a unidic-sized lexicon, 4.4 on the
 * dense synthetic law.  The library picks the LDS tiers of the sweep by it (> 3 = 10 KiB segments, else 8 KiB ones and
 * one more wave per SIMD); exposed for observability.  No reference counterpart.  VBT_TIER_ADAPT=0: not measured, always 0. */
VBT_API int vbt_tokenizer_lattice_density(const vbt_tokenizer* tok, double* candidates_per_byte);
VBT_API void vbt_tokenizer_free(vbt_tokenizer* tok);
VBT_API const vbt_dict* vbt_tokenizer_dictionary(const vbt_tokenizer* tok); /* Tokenizer::dictionary, tokenizer.rs:77 */

/* ---- Worker (per-sentence API, worker.rs:34-75) --------------------------------- */

VBT_API int vbt_worker_new(const vbt_tokenizer* tok, vbt_worker** out);          /* Tokenizer::new_worker */
VBT_API void vbt_worker_free(vbt_worker* w);
VBT_API int vbt_worker_reset_sentence(vbt_worker* w, const char* utf8, size_t len); /* Worker::reset_sentence */
VBT_API int vbt_worker_tokenize(vbt_worker* w);                                   /* Worker::tokenize */
VBT_API uint32_t vbt_worker_num_tokens(const vbt_worker* w);                      /* Worker::num_tokens */
VBT_API int vbt_worker_token(const vbt_worker* w, uint32_t i, vbt_token* out);    /* Worker::token(i) */
/* vbt_worker_reset_sentence fails with VBT_ERR_UTF8 when the bytes are not a Rust `str` (the reference takes &str,
 * worker.rs:34); the worker then holds the empty sentence. */
/* vbt_worker_tokenize costs no launch in steady state: a resident one-wavefront kernel polls a doorbell in the worker's pinned host block,
 * reads the text out of it and writes the token records back into it (no copy engine, no allocation); the call returns when the
 * kernel's status word has landed.  The kernel leaves after ~2 ms without a call (VBT_WORKER_IDLE_POLLS) and, so that it never holds
 * the device against other threads' synchronising calls, after VBT_WORKER_MAX_SERVED (4096) sentences; the next call starts it again.  A kernel
 * that answers late (a busy GPU, a profiler) is waited for up to 5 s, then told to leave; only a failing stream is an error.
 * Sentences a single wavefront cannot take (longer than ~2500 characters, a dictionary word of more
 * than 64 characters, ...) and workers that count connection ids go through the batch pipeline instead.
 * vbt_worker_path_stats: sentences served by the single launch / by the batch pipeline so far. */
VBT_API int vbt_worker_path_stats(const vbt_worker* w, uint64_t* fast, uint64_t* slow);
/* The reference's calling pattern, timed inside the library (tokenize/src/main.rs:78-82, benchmark/src/main.rs:57-61): for each
 * of the n sentences reset_sentence -> tokenize -> num_tokens -> token(i) for every token, `rounds` passes; wall seconds and the
 * number of tokens seen. */
VBT_API int vbt_worker_loop_benchmark(vbt_worker* w, const uint8_t* text, const uint64_t* offsets, uint64_t n, uint32_t rounds,
                                      double* seconds, uint64_t* tokens);
/* Worker::init_connid_counter, worker.rs:77-84 (ConnIdCounter::new, mapper.rs:94-99): zeroed counters */
VBT_API int vbt_worker_init_connid_counter(vbt_worker* w);
/* Worker::update_connid_counts, worker.rs:86-93: adds Lattice::add_connid_counts (lattice.rs:170-183) of the last
 * vbt_worker_tokenize call.  VBT_ERR_INVALID_STATE where the reference panics (no init_connid_counter). */
VBT_API int vbt_worker_update_connid_counts(vbt_worker* w);
/* The raw counters: lid[num_left], rid[num_right]. */
VBT_API int vbt_worker_connid_counts(const vbt_worker* w, uint64_t* lid, uint64_t* rid);
/* Worker::compute_connid_probs, worker.rs:95-103 (ConnIdCounter::compute_probs, mapper.rs:108-146): per side the
 * (id, count / sum) pairs without id 0, sorted by probability descending, then id ascending -- the content of the
 * reference's *.lmap / *.rmap files.  lid_* hold num_left - 1 entries, rid_* num_right - 1. */
VBT_API int vbt_worker_compute_connid_probs(const vbt_worker* w, uint32_t* lid_ids, double* lid_probs, uint32_t* rid_ids,
                                            double* rid_probs);
/* The same computation for one side of any counter array (e.g. vbt_workspace_connid_counts): n - 1 entries out. */
VBT_API int vbt_connid_probs(const uint64_t* counts, size_t n, uint32_t* ids, double* probs);

/* ---- Batched host API (new: many sentences per call) ---------------------------- */

/* The 3-call loop of tokenize/src/main.rs:78-82 over n sentences: sentence s is
 * text[offsets[s] .. offsets[s+1]). Copies text to the device, runs the kernels,
 * copies token records back (the GPU's SDMA engines, into a pinned block sized to the result). The batch keeps its own copy of the text.
 * Every sentence must be valid UTF-8 (a Rust `str`): otherwise VBT_ERR_UTF8 and no batch.
 * ONE call is a pipeline (tokenize/src/main.rs:76-95 is a single-threaded caller): on a single-device tokenizer a lone caller's batch of
 * 4 MiB or more is cut at sentence borders into VBT_H2H_CHUNKS (default 5, 1 = off) chunks that rotate through three chunk-sized
 * workspaces -- the copy in and the copy out of neighbouring chunks run on the SDMA engines next to the kernels of the chunk in
 * between, into ONE result block (40 M sentences/s for one call from one thread on the headline workload; 20 M unpipelined).  The
 * tokenizer's first batch runs unpipelined (it sets the tokens-per-KiB estimate the result block of a pipelined call is sized by; a
 * batch that outgrows the estimate is redone unpipelined).  Results are the same arrays either way.
 * Thread-safe per tokenizer: each call takes workspaces (device scratch + staging + stream) from the tokenizer's
 * pool and returns them, so steady-state calls do no device allocation (vbt_tokenizer_pool_stats); batches pushed from
 * several host threads overlap their copies with each other's kernels (4-8 threads reach 62-66 M sentences/s; such calls are not
 * cut into chunks: only a caller that has been alone for its last two calls is).
 * The pools keep idle workspaces (~400 B of device memory per byte of text of the batch they were sized for) and pinned
 * blocks for reuse, at most VBT_POOL_MAX_MB=<device MB>[,<pinned MB>] of each (default: a quarter of the GPU's memory -- 72 GiB on
 * an MI355X -- and 8192 MB of pinned memory; what would exceed it is released instead of pooled, and a caller whose workspace
 * never fits re-allocates it on every call); vbt_tokenizer_trim_pool releases everything idle now. */
VBT_API int vbt_tokenize_batch(const vbt_tokenizer* tok, const uint8_t* text, const uint64_t* offsets, uint64_t n,
                               vbt_batch** out);
VBT_API int vbt_tokenizer_trim_pool(const vbt_tokenizer* tok);
VBT_API int vbt_tokenizer_pool_stats(const vbt_tokenizer* tok, uint64_t* created, uint64_t* reused, uint64_t* idle);
VBT_API void vbt_batch_free(vbt_batch* b);
VBT_API uint64_t vbt_batch_num_sentences(const vbt_batch* b);
VBT_API uint64_t vbt_batch_total_tokens(const vbt_batch* b);
VBT_API uint32_t vbt_batch_num_tokens(const vbt_batch* b, uint64_t sentence);
VBT_API int vbt_batch_token(const vbt_batch* b, uint64_t sentence, uint32_t i, vbt_token* out);
/* Raw records of one sentence (num_tokens of them, in sentence order). */
VBT_API const vbt_token_rec* vbt_batch_records(const vbt_batch* b, uint64_t sentence);
/* Whole-batch views: sentence s owns tokens[tok_off[s] .. tok_off[s] + tok_cnt[s]). */
VBT_API int vbt_batch_arrays(const vbt_batch* b, const vbt_token_rec** tokens, const uint32_t** tok_off,
                             const uint32_t** tok_cnt);
/* Byte-identical output of the `tokenize` CLI for the whole batch (tokenize/src/main.rs:83-127).
 * *out belongs to the library: release it ONLY with vbt_free (never free(): the pointer does not start a malloc block).  Rendered by up
 * to VBT_FORMAT_THREADS host threads (default: the host's cores, at most 64) in two passes over chunks of sentences: exact sizes,
 * then every chunk in place. */
VBT_API int vbt_batch_format(const vbt_batch* b, int mode, char** out, size_t* len);
/* Releases a buffer handed out by vbt_batch_format / vbt_dict_write.  A pointer that is not a live buffer of this library (freed
 * already, or from somewhere else) is ignored.  Big buffers are kept for the next call (at most 4 / 512 MiB per process) until
 * vbt_tokenizer_trim_pool or vbt_tokenizer_free. */
VBT_API void vbt_free(void* p);
/* Host text in -> wakati text out (tokenize/src/main.rs:96-103: the surfaces of a sentence joined by ' ', then '\n'; "\n" for a
 * sentence without tokens; the lines of the n sentences back to back), rendered ON THE DEVICE: the same bytes as vbt_tokenize_batch +
 * vbt_batch_format(VBT_FORMAT_WAKATI), but no token records are packed or copied and no host thread formats anything -- the text goes
 * in, two kernels behind the sweeps write the lines (vbt_workspace_set_wakati), the 8-byte total comes back and exactly that many
 * bytes are copied into a pinned block (by the SDMA engine vbt_tokenize_batch uses): about a quarter of the bytes the records are.
 * *out is released ONLY with vbt_free, like vbt_batch_format's; line_off (optional): n + 1 entries, line s is
 * out[line_off[s] .. line_off[s + 1]), line_off[n] = *len.  Input contract and error codes as vbt_tokenize_batch (VBT_ERR_UTF8, ...).
 * One unpipelined call on a pooled workspace; thread-safe per tokenizer.  A multi-device tokenizer (vbt_tokenizer_new_multi with more than
 * one device) is refused with VBT_ERR_UNSUPPORTED: sharded rendering is not implemented. */
VBT_API int vbt_tokenize_wakati(const vbt_tokenizer* tok, const uint8_t* text, const uint64_t* offsets, uint64_t n,
                                char** out, size_t* len, uint64_t* line_off);
/* Host text in -> MeCab-format text out (tokenize/src/main.rs:83-95: "surface \t feature \n" per token, then "EOS\n"; "EOS\n" alone
 * for a sentence without tokens; the lines of the n sentences back to back), rendered ON THE DEVICE: the same bytes as
 * vbt_tokenize_batch + vbt_batch_format(VBT_FORMAT_MECAB), but no token records are packed or copied and no host thread formats
 * anything -- the feature strings are a table of the device image (uploaded at the first call), kernels behind the sweeps write the
 * lines (vbt_workspace_set_mecab), 16 bytes come back and exactly *len bytes are copied into a pinned block by the SDMA engine.
 * The input does not bound this output: the first capacity is taken from the largest output-per-input ratio this tokenizer has seen
 * (+ 1/8 + 4 n; 8 x bytes + 4 n before any batch; VBT_MECAB_FIRST_CAP = bytes in the environment, read per call, overrides it), and
 * a batch that does not fit is rendered ONCE more into a buffer of the exact size (vbt_workspace_render_again), not tokenized again.
 * *out is released ONLY with vbt_free; line_off (optional): n + 1 entries, line_off[n] = *len.  Input contract and error codes as
 * vbt_tokenize_batch.  One unpipelined call on a pooled workspace; thread-safe per tokenizer.  A multi-device tokenizer is refused
 * with VBT_ERR_UNSUPPORTED: sharded rendering is not implemented. */
VBT_API int vbt_tokenize_mecab(const vbt_tokenizer* tok, const uint8_t* text, const uint64_t* offsets, uint64_t n,
                               char** out, size_t* len, uint64_t* line_off);
/* Host text in -> detail text out (tokenize/src/main.rs:108-123: per token "surface \t feature \tlex_type=System|User|Unknown
 * \tleft_id=N \tright_id=N \tword_cost=N \ttotal_cost=N \n", then "EOS\n"), rendered ON THE DEVICE: the same bytes as
 * vbt_tokenize_batch + vbt_batch_format(VBT_FORMAT_DETAIL), with the contract of vbt_tokenize_mecab in everything -- one unpipelined
 * call on a pooled workspace, the first capacity from the largest output-per-input ratio seen FOR THIS MODE (+ 1/8 + 4 n; 16 x bytes
 * + 4 n before any batch; VBT_DETAIL_FIRST_CAP = bytes in the environment, read per call, overrides it -- VBT_MECAB_FIRST_CAP does
 * not apply here), at most one re-render, *out released ONLY with vbt_free, VBT_ERR_UNSUPPORTED for a multi-device tokenizer.  The
 * ids printed are the dictionary's, from a word-parameter table of the device image uploaded at the first call. */
VBT_API int vbt_tokenize_detail(const vbt_tokenizer* tok, const uint8_t* text, const uint64_t* offsets, uint64_t n,
                                char** out, size_t* len, uint64_t* line_off);
/* User-defined output formats, rendered ON THE DEVICE (MeCab's --node-format / --unk-format / --bos-format / --eos-format, -F -U -B
 * -E): per sentence the bos bytes, one expansion of `node` per token -- of `unk` for a word of the unknown lexicon -- and the eos
 * bytes; a sentence without tokens is bos + eos.  unk == NULL: = node; bos == NULL: ""; eos == NULL: "EOS\n".  Directives, with MeCab's
 * meanings: %m the surface; %H the whole feature string as stored (what vbt_tokenize_mecab prints); %f[i] CSV field i (from 0) of the
 * feature, unquoted as utils::parse_csv_row (utils.rs:40-61) yields it, nothing when the feature has no field i; %f[i,j,..] those
 * fields joined by ',' (an absent one is an empty string between the commas); %F<c>[i,j,..] those fields joined by the byte <c>,
 * SKIPPING the fields that are absent or exactly "*"; %pw and %c the word cost, %pc the total cost, %phl / %phr the DICTIONARY's left
 * / right id (never the device's renumbered ids); %ps %pe %pl the token's start byte, end byte and byte length in its sentence; %s 0
 * for a system or user word, 1 for an unknown word; %% a '%'.  Escapes in all four strings: \0 \a \b \t \n \v \f \r \\ (the
 * control bytes themselves are taken as they are).  bos and eos take literals, escapes and %% only.  Limits: 32 ops per string --
 * a directive is one op, every index of a %f / %F list one of its own, every run of literal bytes one --, 16 distinct field indices
 * per format, field index <= 255, 256 literal bytes per string.  Anything else -- an unknown directive or escape, an unterminated
 * '[', an empty index list, a directive in bos or eos -- is VBT_ERR_INVALID_ARGUMENT with a message that names the string and the
 * position.  Out of scope: %pC, %pP and the other lattice-level directives.
 * vbt_format_check: the validation alone -- pure host code, no device; err
 *   (optional, errcap bytes) receives the message.
 * vbt_format_new: compiles the four strings for `tok`, which has to outlive the format.  The device side -- a field index {offset,
 *   length} per word and wanted field, cut out of the feature table in device memory BY A KERNEL (no host pass over the feature
 *   text; the few words with a doubled quote or bytes behind a closing quote are parsed by the host into a side blob) -- is built at
 *   the first use, is independent of the renumbering of the connection ids, and is freed by vbt_format_free.
 * vbt_tokenize_format: vbt_tokenize_mecab's contract in everything -- one unpipelined call, the first capacity from the largest
 *   output-per-input ratio seen FOR THIS FORMAT OBJECT (+ 1/8 + 4 n; 8 x bytes + 4 n before any batch; VBT_FORMAT_FIRST_CAP = bytes in
 *   the environment, read per call, overrides it), at most one re-render, *out released ONLY with vbt_free, VBT_ERR_UNSUPPORTED for
 *   a multi-device tokenizer (sharded rendering is not implemented).  vbt_tokenize_stream does not take a format. */
typedef struct vbt_format vbt_format;
VBT_API int vbt_format_check(const char* node, const char* unk, const char* bos, const char* eos, char* err, size_t errcap);
VBT_API int vbt_format_new(const vbt_tokenizer* tok, const char* node, const char* unk, const char* bos, const char* eos, vbt_format** out);
VBT_API void vbt_format_free(vbt_format* fmt);
VBT_API int vbt_tokenize_format(const vbt_tokenizer* tok, const vbt_format* fmt, const uint8_t* text, const uint64_t* offsets, uint64_t n,
                                char** out, size_t* len, uint64_t* line_off);
/* Raw bytes in -> sentences out, the lines cut ON THE DEVICE (split.hip) with the semantics of BufRead::lines(), which the
 * reference's CLI reads its input with (tokenize/src/main.rs:78-80): a line ends at '\n'; ONE '\r' directly in front of that '\n' goes
 * with it; every other '\r' is text (a lone one, the first of "\r\r\n", the last byte of an unterminated last line); an empty line is
 * a sentence of length 0; a trailing '\n' opens no further sentence.  What follows the last '\n' is the tail: with final != 0 a tail
 * that is not empty is the last sentence and *consumed = len; with final == 0 the tail is left to the caller -- *consumed is the index
 * behind the last '\n' (0 and *n = 0 when there is none), and the next call starts with raw + *consumed in front of what was read
 * since.  *text = the sentences back to back without their terminators, *offsets = n + 1 byte offsets into it (offsets[0] = 0): what
 * vbt_tokenize_batch and -- on the device -- vbt_tokenize_batch_device take.  Both are released ONLY with vbt_free.  The bytes are
 * not checked for UTF-8 here (the tokenize calls do that).  Three kernels over tiles of VBT_SPLIT_TILE bytes -- count, scan of the
 * tiles' counts, scatter -- none of which waits for another workgroup.  len >= 4 GiB: VBT_ERR_INVALID_ARGUMENT; a multi-device
 * tokenizer: VBT_ERR_UNSUPPORTED; len == 0 launches nothing. */
#define VBT_SPLIT_TILE 16384
VBT_API int vbt_split_lines(const vbt_tokenizer* tok, const uint8_t* raw, size_t len, int final, uint8_t** text,
                            uint64_t** offsets /* n + 1 */, uint64_t* n, size_t* consumed);
/* Raw bytes in -> rendered text out (mode = VBT_FORMAT_MECAB | VBT_FORMAT_WAKATI | VBT_FORMAT_DETAIL): vbt_split_lines in front of
 * vbt_tokenize_mecab / _wakati / _detail without the sentences ever visiting the host -- the raw bytes go to the device in one copy,
 * 16 bytes come back ({n, consumed, bytes of text}: the call picks its pooled workspace by them), the scatter kernel writes the
 * text and the offsets where the tokenizer reads them, and everything behind is the text call of that mode (capacity protocol, at
 * most one re-render, *out released ONLY with vbt_free).  *n = sentences rendered, *consumed as vbt_split_lines.  Errors as there, and
 * VBT_ERR_UTF8 naming the line (counted from 0 within this call) for text that is not UTF-8. */
VBT_API int vbt_tokenize_stream(const vbt_tokenizer* tok, int mode, const uint8_t* raw, size_t len, int final, char** out,
                                size_t* out_len, uint64_t* n, size_t* consumed);

/* ---- N-best (new: MeCab's -N; the reference keeps one best path, lattice.rs:129-151) -------- */

typedef struct vbt_nbest vbt_nbest;
/* Host text in -> the `nbest` cheapest paths of every sentence out, in host memory (MeCab's -N; no reference counterpart: the sweep
 * of lattice.rs:129-151 keeps one (min_cost, back pointer) per node, the kernel behind this call keeps `nbest` sorted entries per
 * node and merges them -- nbest.hip).  The lattice is the one vbt_tokenize_batch takes its path from (same candidates
 * in the same insertion order, ignore_space, max_grouping_len, user lexicon, unknown words; two homographs of a surface are two
 * nodes), the cost of a path is the 1-best's i32 arithmetic (word_cost + connection per node + the connection to EOS), and the
 * paths come in a total order: lower cost first; on equal cost the two paths are compared from EOS backwards and, at the first
 * node where they differ, the node inserted LATER into its end list comes first -- the `<=` of lattice.rs:141-146 applied
 * recursively, so path 0 is exactly vbt_tokenize_batch's, record by record.  A sentence yields min(nbest, its paths) paths: an
 * empty sentence none (worker.rs:50-52), a sentence of skipped spaces one path of no tokens.  total_cost of a record is the cost
 * accumulated ALONG ITS PATH.  Where an i32 sum wraps the order is that of the wrapped values, entry by entry.
 * nbest outside 1 .. 16: VBT_ERR_INVALID_ARGUMENT; a multi-device tokenizer: VBT_ERR_UNSUPPORTED; input contract and the other
 * error codes as vbt_tokenize_batch.  The batch is cut at sentence borders into chunks whose record staging -- nbest x (bytes + 24 x
 * sentences) records of 24 bytes -- stays within 768 MiB (the workspace rounds capacities up to powers of two and holds as much
 * again for the packed records, + at most 1 GiB of scratch for the lattices that outgrow LDS); the workspace is kept by the
 * tokenizer between calls, and calls on one tokenizer take turns.  VBT_NBEST_LDS_KB (read when the tokenizer is created, default
 * 32, at most 64; 0 = every lattice in global memory) is the LDS a wavefront's lattice may use. */
VBT_API int vbt_tokenize_nbest(const vbt_tokenizer* tok, const uint8_t* text, const uint64_t* offsets, uint64_t n,
                               uint32_t nbest, vbt_nbest** out);
VBT_API void vbt_nbest_free(vbt_nbest* r);                                /* releases a result of vbt_tokenize_nbest (MeCab's -N; lattice.rs:129-151) */
VBT_API uint64_t vbt_nbest_num_sentences(const vbt_nbest* r);             /* sentences of the call (MeCab's -N; lattice.rs:129-151) */
/* Paths of sentence s, at most the call's nbest (MeCab's -N; lattice.rs:129-151). */
VBT_API uint32_t vbt_nbest_num_paths(const vbt_nbest* r, uint64_t sentence);
/* Cost of path `rank` of sentence s: the total_cost of EOS along it (MeCab's -N; lattice.rs:129-151).  Ranks ascend by the order above. */
VBT_API int vbt_nbest_path_cost(const vbt_nbest* r, uint64_t sentence, uint32_t rank, int32_t* cost);
/* Its records, in sentence order, and their number (MeCab's -N; lattice.rs:129-151); the pointer lives until vbt_nbest_free. */
VBT_API int vbt_nbest_path_records(const vbt_nbest* r, uint64_t sentence, uint32_t rank, const vbt_token_rec** records,
                                   uint32_t* count);
/* The four raw arrays (MeCab's -N; lattice.rs:129-151): sentence s owns the paths [path_off[s], path_off[s + 1]) (n + 1 entries),
 * path p the records tokens[tok_off[p] .. tok_off[p + 1]) (paths + 1 entries) and the cost path_cost[p]. */
VBT_API int vbt_nbest_arrays(const vbt_nbest* r, const uint64_t** path_off, const uint64_t** tok_off,
                             const int32_t** path_cost, const vbt_token_rec** tokens);
/* Sentences of the call whose lattice did not fit the LDS tier and was built in global memory (observability; MeCab's -N; lattice.rs:129-151). */
VBT_API uint64_t vbt_nbest_slab_sentences(const vbt_nbest* r);

/* ---- Lattice marginals (new: MeCab's -m / -l 2 with -t; the reference keeps one best path, lattice.rs:129-151) -------- */

typedef struct vbt_marginal vbt_marginal;
/* One reported lattice node: its span, its word (word_idx as in vbt_token_rec) and the summed probability of the paths through it. */
typedef struct vbt_marginal_node {
    uint32_t start_char, end_char, start_byte, end_byte;
    uint32_t word_idx;
    uint32_t reserved; /* 0 */
    double prob;
} vbt_marginal_node;
/* Host text in -> the posterior probability of every lattice node out, in host memory (a forward-backward sweep in float64:
 * marginal.hip).  The lattice is the one vbt_tokenize_batch takes its path from (same candidates in the same
 * insertion order, unknown words, user lexicon, ignore_space, max_grouping_len, the same steps with the EOS step and the "input ends
 * with spaces" rule).  The cost of a path is the EXACT integer sum of its word costs and connection costs, the connection to EOS
 * included -- it does not wrap as the 1-best's i32 accumulator does.  P(path) = exp(-cost / temperature) / Z, `temperature` in cost
 * units (MeCab's -t theta with a dictionary cost factor f corresponds to temperature = f / theta); log_z = log of the sum of
 * exp(-cost / temperature) over all paths; a node's prob = the summed probability of the paths through it.  A node is reported iff
 * its prob is positive in float64 and >= min_prob -- dead ends (nothing follows them, or nothing reaches them) drop out by that
 * rule -- and the nodes of a sentence come in lattice order: by start position, then candidate insertion order.  An empty sentence,
 * and one of spaces only under ignore_space, has no nodes and log_z = 0.
 * temperature not finite or <= 0, min_prob outside [0, 1] or NaN: VBT_ERR_INVALID_ARGUMENT; a multi-device tokenizer:
 * VBT_ERR_UNSUPPORTED; input contract and the other error codes as vbt_tokenize_nbest.  The node count of a sentence is not bounded
 * by its bytes: the node staging starts at 4 records per byte + 64 per sentence (the batch is cut at sentence borders into chunks
 * that keep this within 768 MiB), sentences that find it full are run again with a staging of the size the run asked for, and a
 * node list is never truncated.  The workspace is kept by the tokenizer between calls, and calls on one tokenizer take turns.
 * VBT_MARGINAL_LDS_KB (read when the tokenizer is created, default 32, at most 64; 0 = every lattice in global memory) is the LDS
 * a wavefront's lattice may use. */
VBT_API int vbt_tokenize_marginal(const vbt_tokenizer* tok, const uint8_t* text, const uint64_t* offsets, uint64_t n,
                                  double temperature, double min_prob, vbt_marginal** out);
VBT_API void vbt_marginal_free(vbt_marginal* r);                          /* releases a result of vbt_tokenize_marginal (MeCab's -m; lattice.rs:129-151) */
VBT_API uint64_t vbt_marginal_num_sentences(const vbt_marginal* r);       /* sentences of the call (MeCab's -m; lattice.rs:129-151) */
/* log Z of sentence s (MeCab's -m; lattice.rs:129-151). */
VBT_API int vbt_marginal_log_z(const vbt_marginal* r, uint64_t sentence, double* log_z);
/* Its reported nodes, in lattice order, and their number (MeCab's -m; lattice.rs:129-151); the pointer lives until vbt_marginal_free. */
VBT_API int vbt_marginal_nodes(const vbt_marginal* r, uint64_t sentence, const vbt_marginal_node** nodes, uint64_t* count);
/* The three raw arrays (MeCab's -m; lattice.rs:129-151): sentence s owns the nodes [node_off[s], node_off[s + 1]) (n + 1 entries)
 * and log_z[s] (n entries). */
VBT_API int vbt_marginal_arrays(const vbt_marginal* r, const uint64_t** node_off, const double** log_z,
                                const vbt_marginal_node** nodes);
/* Sentences of the call whose lattice did not fit the LDS tier and was built in global memory (observability; MeCab's -m; lattice.rs:129-151). */
VBT_API uint64_t vbt_marginal_slab_sentences(const vbt_marginal* r);

/* ---- Sampled segmentations (new: forward filtering / backward sampling over the lattice of the marginals) -------- */

typedef struct vbt_sample vbt_sample;
/* Host text in -> n_samples whole paths per sentence out, in host memory: independent draws, with repetition, from
 * P(path) = exp(-cost / temperature) / Z over the lattice vbt_tokenize_marginal states (same candidates in insertion order, unknown
 * words, user lexicon, ignore_space, max_grouping_len, the EOS step; sample.hip).  The cost of a path is the EXACT
 * integer sum and does not wrap: path_cost is int64.  total_cost inside a record stays i32: it is accumulated along the path and
 * wraps as vbt_tokenize_nbest's does.  A sentence with a path yields exactly n_samples paths; an empty sentence none; a sentence of
 * skipped spaces only n_samples paths of no tokens with log_z = 0.  log_z = alpha(EOS), as vbt_tokenize_marginal reports it.
 *
 * The draw is part of the contract.  Sample r of the sentence with index s -- counted over the whole call, not within a chunk --
 * walks from EOS to BOS.  Draw number t (0 at EOS, + 1 per token) chooses the predecessor of the current node c among the np
 * entries of c's predecessor end list, in end-list (= insertion) order, with weights p_j = exp(alpha_j - conn(j, c) / T - L_c),
 * L_c = LSE_j(alpha_j - conn(j, c) / T) (in the kernel L_c = alpha_c + w_c / T); a slot with alpha = -inf has weight 0.  The chosen
 * j is the smallest one with sum_{i<=j} p_i > u x sum_i p_i -- the right-hand sum is the computed one, not 1 -- and if rounding
 * leaves none, the last j of positive weight.  (The kernel adds in chunks of ceil(np / 16) consecutive entries and scans the 16
 * chunk sums; that order is fixed, so a result is reproducible bit by bit, and differs from the plain running sum only where u x
 * sum lies within rounding of a boundary.)  u = (x + 0.5) x 2^-32, x = word 0 of Philox4x32-10 (10 rounds, multipliers 0xD2511F53
 * and 0xCD9E8D57, key increments 0x9E3779B9 and 0xBB67AE85) with counter (lo32(s), hi32(s), r, t) and key (lo32(seed), hi32(seed)).
 * A result depends on the text, the dictionary, the temperature, n_samples, seed and s only: not on chunking, the tier a lattice
 * ran in, staging blocks or the renumbered device image.
 *
 * temperature not finite or <= 0, n_samples outside 1 .. 64: VBT_ERR_INVALID_ARGUMENT; a multi-device tokenizer:
 * VBT_ERR_UNSUPPORTED; input contract and the other error codes as vbt_tokenize_nbest.  The batch is cut at sentence borders into
 * chunks whose record staging -- n_samples x (bytes + 24 x sentences) records of 24 bytes -- stays within 768 MiB; nothing can
 * overflow.  VBT_MARGINAL_LDS_KB / VBT_MARGINAL_STAGE_KB apply as for vbt_tokenize_marginal.  The workspace is kept by the tokenizer
 * between calls, and calls on one tokenizer take turns. */
VBT_API int vbt_tokenize_sample(const vbt_tokenizer* tok, const uint8_t* text, const uint64_t* offsets, uint64_t n,
                                double temperature, uint32_t n_samples, uint64_t seed, vbt_sample** out);
VBT_API void vbt_sample_free(vbt_sample* r);                              /* releases a result of vbt_tokenize_sample */
VBT_API uint64_t vbt_sample_num_sentences(const vbt_sample* r);           /* sentences of the call */
/* Paths of sentence s: the call's n_samples, or 0 for an empty sentence. */
VBT_API uint32_t vbt_sample_num_paths(const vbt_sample* r, uint64_t sentence);
/* Cost of sample `rank` of sentence s: the exact sum of its word and connection costs, the connection to EOS included. */
VBT_API int vbt_sample_path_cost(const vbt_sample* r, uint64_t sentence, uint32_t rank, int64_t* cost);
/* Its records, in sentence order, and their number; the pointer lives until vbt_sample_free. */
VBT_API int vbt_sample_path_records(const vbt_sample* r, uint64_t sentence, uint32_t rank, const vbt_token_rec** records,
                                    uint32_t* count);
/* log Z of sentence s. */
VBT_API int vbt_sample_log_z(const vbt_sample* r, uint64_t sentence, double* log_z);
/* The five raw arrays: sentence s owns the paths [path_off[s], path_off[s + 1]) (n + 1 entries) and log_z[s] (n entries), path p
 * the records tokens[tok_off[p] .. tok_off[p + 1]) (paths + 1 entries) and the cost path_cost[p]. */
VBT_API int vbt_sample_arrays(const vbt_sample* r, const uint64_t** path_off, const uint64_t** tok_off,
                              const int64_t** path_cost, const double** log_z, const vbt_token_rec** tokens);
/* Sentences of the call whose lattice did not fit the LDS tier and was built in global memory (observability). */
VBT_API uint64_t vbt_sample_slab_sentences(const vbt_sample* r);

/* ---- Device-resident API (zero-copy; what bench.py times) ------------------------ */

/* A workspace owns the device scratch + output buffers for batches of up to
 * max_sentences sentences / max_bytes bytes of text, and is reused across calls.
 * Footprint: about 400 bytes of device memory per byte of text (candidate records and staged trie hits at 8 slots of
 * 16 bytes per input byte each, token staging + compact tokens at 24 bytes each, per-character records, the fused
 * fallback's scratch) plus ~7 KB per sentence (head room of its node region): ~6.5 GB for the 14 MB / 100k-sentence headline batch, and at most
 * ~0.6 GB of text per workspace on a 288 GB part -- larger corpora are fed as a sequence of batches (the host entry
 * point vbt_tokenize_batch refuses a batch of 4 GiB or more outright; VBT_ERR_DEVICE when the allocation fails). */
VBT_API int vbt_workspace_new(const vbt_tokenizer* tok, uint64_t max_sentences, uint64_t max_bytes, vbt_workspace** out);
VBT_API void vbt_workspace_free(vbt_workspace* ws);
/* Enqueue the tokenization of n sentences on `hip_stream` (a hipStream_t, NULL = default
 * stream). d_text / d_offsets are DEVICE pointers (offsets: n+1 x u64, bytes into d_text;
 * offsets[0] need not be 0: the batch may be a window into a larger text buffer).
 * Asynchronous; results are valid once the stream has been synchronized.
 * Input contract, checked on the device by the first kernel of the call: offsets non-decreasing,
 * offsets[n] - offsets[0] <= total_bytes (<= the workspace's max_bytes, checked on the host), text valid UTF-8
 * with every sentence starting on a character boundary.  A violation skips the batch and shows up as
 * error_flags 8 (offsets) / 16 (UTF-8) in vbt_workspace_stats; results of that call are undefined. */
VBT_API int vbt_tokenize_batch_device(vbt_workspace* ws, const uint8_t* d_text, const uint64_t* d_offsets, uint64_t n,
                                      uint64_t total_bytes, void* hip_stream);
/* Device pointers to the results of the last call:
 *   tokens   : vbt_token_rec[], sentence s occupies [tok_off[s], tok_off[s] + tok_cnt[s])
 *   tok_off  : u32[n]  (allocation order is unspecified; content is deterministic)
 *   tok_cnt  : u32[n]
 *   total    : u32[1]  total tokens written */
VBT_API int vbt_workspace_results(const vbt_workspace* ws, const vbt_token_rec** d_tokens, const uint32_t** d_tok_off,
                                  const uint32_t** d_tok_cnt, const uint32_t** d_total);
/* The final exchange of a multi-GPU job without copy kernels: every later vbt_tokenize_batch_device call of this workspace leaves
 * its results in ONE caller-owned device buffer laid out as a rank's slot of the gather (vibrato_amd/sharding.py; north_star:
 * "RCCL over xGMI only for the final gather"):
 *   [32-byte header {n_sentences u64, n_tokens u32, error flags u32, 0 x 16 bytes}] [tok_off u32 x max_sentences] [tok_cnt u32 x max_sentences] [vbt_token_rec x n_tokens]
 * -- tok_cnt written by the sweep, tok_off and the records by the packing kernel, the header with its total -- so the collective
 * (ncclSend / all-gather of the slot) starts from what the tokenizer wrote.  d_slot: 8-byte aligned device memory of slot_bytes >=
 * 32 + 8 max_sentences + 24 x (tokens of the largest batch); a batch whose tokens do not fit sets error flag 1 -- in the workspace's
 * statistics AND in the header's flags word, whose n_tokens is then the number of records the slot holds (a consumer of gathered slots
 * sees nothing else of the rank that wrote one).  d_slot = NULL:
 * back to the workspace's own buffers.  vbt_workspace_results then points into the slot.  The caller alternates two slots to
 * overlap the gather of batch k with the kernels of batch k + 1. */
VBT_API int vbt_workspace_set_packed_output(vbt_workspace* ws, void* d_slot, uint64_t slot_bytes, uint64_t max_sentences);
/* Wakati output on the device.  While enabled, every vbt_tokenize_batch_device call of this workspace also renders the segmented
 * text of its batch -- line s = the surfaces of sentence s joined by ' ', then '\n' -- into a buffer the workspace owns (allocated
 * when the mode is first enabled: 2 max_bytes + max_sentences bytes, the bound of bytes + tokens + sentences), straight from the
 * sweeps' per-sentence staging: the token records are NOT packed (vbt_workspace_results is then undefined except tok_cnt and the
 * total) unless keep_records is set.  A wave renders a sentence VBT_WAKATI_ROUND tokens at a time.
 * enabled: 0 = off, 1 = on, a value > 1 = on with the output limited to that many bytes (callers that budget device memory, tests):
 * a line that would end beyond the limit sets error flag 32 and is not written, the lines in front of it are.  The 64 bytes behind
 * the capacity belong to the buffer and are never written.
 * vbt_workspace_wakati: d_out = the lines back to back, d_line_off = u64[n + 1] byte offsets of the lines, d_line_off[n] = bytes
 * written; device pointers, valid once the stream of the call has been synchronized. */
#define VBT_WAKATI_ROUND 256
VBT_API int vbt_workspace_set_wakati(vbt_workspace* ws, int enabled, int keep_records);
VBT_API int vbt_workspace_wakati(const vbt_workspace* ws, const uint8_t** d_out, const uint64_t** d_line_off /* n + 1 */);
/* MeCab-format output on the device (tokenize/src/main.rs:83-95).  While enabled, every vbt_tokenize_batch_device call of this
 * workspace also renders the MeCab-format text of its batch -- per token "surface \t feature \n", per sentence "EOS\n" -- straight
 * from the sweeps' per-sentence staging and the feature table of the device image (uploaded when the first workspace of a tokenizer
 * enables the mode); the token records are NOT packed unless keep_records is set.  One text mode at a time: enabling this mode on a
 * workspace in wakati mode, or the reverse, is VBT_ERR_INVALID_ARGUMENT.  A wave renders a sentence VBT_MECAB_ROUND tokens at a time.
 * cap_bytes (> 0 when enabling): the capacity of the output buffer, which the input does NOT bound (a token adds its feature string,
 * 40-150 bytes with the usual dictionaries).  The buffer is allocated, or replaced by a larger one, when more is asked for than it
 * holds.  A line that would end beyond the capacity (or a line of 4 GiB and more) sets error flag 32 -- the text output capacity flag
 * of both text modes -- and is not written, the lines in front of it are; d_line_off[n] is the exact number of bytes the batch needs
 * either way.  The 64 bytes behind the capacity belong to the buffer and are never written.
 * vbt_workspace_mecab: as vbt_workspace_wakati (the pointer changes when the buffer is replaced).
 * vbt_workspace_render_again (tokenize/src/main.rs:83-95): valid after a call in this mode until the next one, the batch's d_text /
 * d_offsets still in place: takes flag 32 back on `hip_stream` and renders the lines once more -- after vbt_workspace_set_mecab with
 * a larger cap_bytes, growing the buffer costs one render kernel, not a second tokenization. */
#define VBT_MECAB_ROUND 128
VBT_API int vbt_workspace_set_mecab(vbt_workspace* ws, int enabled, int keep_records, uint64_t cap_bytes);
VBT_API int vbt_workspace_mecab(const vbt_workspace* ws, const uint8_t** d_out, const uint64_t** d_line_off /* n + 1 */);
VBT_API int vbt_workspace_render_again(vbt_workspace* ws, void* hip_stream);
/* Detail output on the device (tokenize/src/main.rs:108-123).  As MeCab mode, with every token's line extended by "\tlex_type=..
 * \tleft_id=.. \tright_id=.. \tword_cost=.. \ttotal_cost=.." in front of its newline: the ids and the word cost are the
 * dictionary's (a word-parameter table of the device image, uploaded when the first workspace of a tokenizer enables the mode),
 * the decimal fields are converted on the device.  cap_bytes, flag 32, d_line_off[n], the 64-byte pad and vbt_workspace_render_again
 * (tokenize/src/main.rs:108-123: it serves whichever of the two modes the last call used) are MeCab mode's; the two modes share one
 * output buffer.  One text mode at a time among the three: enabling one while another is on is VBT_ERR_INVALID_ARGUMENT.  A wave
 * renders a sentence VBT_DETAIL_ROUND tokens at a time.
 * vbt_workspace_detail (tokenize/src/main.rs:108-123): as vbt_workspace_mecab. */
#define VBT_DETAIL_ROUND 64
VBT_API int vbt_workspace_set_detail(vbt_workspace* ws, int enabled, int keep_records, uint64_t cap_bytes);
VBT_API int vbt_workspace_detail(const vbt_workspace* ws, const uint8_t** d_out, const uint64_t** d_line_off /* n + 1 */);
/* Output in a compiled format on the device (vbt_format_new).  As MeCab mode -- cap_bytes, flag 32, d_line_off[n], the 64-byte pad
 * and vbt_workspace_render_again (it serves whichever mode the last call used) are MeCab mode's, the modes share
 * one output buffer -- with the lines of `fmt` (NULL: the mode is switched off), which has to belong to the workspace's tokenizer and
 * to outlive the calls that use it.  One text mode at a time among the four: enabling one while another is on is
 * VBT_ERR_INVALID_ARGUMENT.  A wave renders a sentence VBT_FORMAT_ROUND tokens at a time.
 * vbt_workspace_format: as vbt_workspace_mecab. */
#define VBT_FORMAT_ROUND 64
VBT_API int vbt_workspace_set_format(vbt_workspace* ws, const vbt_format* fmt, int keep_records, uint64_t cap_bytes);
VBT_API int vbt_workspace_format(const vbt_workspace* ws, const uint8_t** d_out, const uint64_t** d_line_off /* n + 1 */);
/* Per-call statistics (synchronizes the stream of the last call): how many sentences were filed
 * in the LDS tiers sentences are routed to up front -- the lean tier and the segment tier (n_tier0) --, in the escape tiers behind
 * them (n_tier1: what a sweep passed on) and in the list of the global-memory fallback kernel (n_tier2; a re-routed sentence is
 * counted in every list it was filed in), tokens
 * written, device error flags (1 = token buffer full, 2 = scratch exhausted, 4 = sentence too
 * long, 8 = bad offsets, 16 = invalid UTF-8, 32 = a line of the text output -- wakati, MeCab or detail mode -- did not fit the output buffer) and, with timing enabled, the hipEvent-measured durations (ms, on the launch stream) of the
 * input check and the candidate generators (ms_tier0: validate_batch, gen_candidates, build_lists, the gen_long levels), of the
 * lattice sweeps from their fork to their join (ms_tier12) and of what follows -- the global-memory fallback launch and the packing
 * of the token records and, in wakati, MeCab or detail mode, the three kernels that render the lines (ms_pack). */
typedef struct vbt_call_stats {
    uint64_t n_sentences, n_tier0, n_tier1, n_tier2, n_tokens;
    uint32_t error_flags;
    float ms_tier0, ms_tier12, ms_pack;
} vbt_call_stats;
VBT_API int vbt_workspace_set_timing(vbt_workspace* ws, int enabled);
/* Worker::init_connid_counter / update_connid_counts (worker.rs:77-93, Lattice::add_connid_counts lattice.rs:170-183):
 * while enabled, every batch adds, for each adjacent (left node, right node) pair of each lattice, 1 to
 * lid[right_node.left_id] and rid[left_node.right_id] (every sentence exactly once, whichever kernel ends up sweeping
 * it).  vbt_workspace_connid_counts copies the totals (num_left / num_right u64). */
VBT_API int vbt_workspace_count_connids(vbt_workspace* ws, int enabled);
VBT_API int vbt_workspace_connid_counts(vbt_workspace* ws, uint64_t* lid, uint64_t* rid, int reset);
/* Developer aid: per-phase shader-clock cycles summed over all sentences since the last reset
 * (enabled by VBT_PROFILE=1 in the environment when the workspace is created). out[0..7] =
 * decode, count, fill, end lists, pre-pass, pass records, recurrence, emit; out[8] = sentences,
 * out[9] = lattice steps, out[10] = lattice passes, out[11] = lattice candidates. */
VBT_API int vbt_workspace_profile(vbt_workspace* ws, uint64_t out[12], int reset);
VBT_API int vbt_workspace_stats(vbt_workspace* ws, vbt_call_stats* out);

#ifdef __cplusplus
}
#endif
#endif /* VIBRATO_HIP_H */
