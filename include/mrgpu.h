/*
 * mrgpu.h -- C ABI of libmrgpu.so, the MI355X (gfx950) engine for the Freebirdgo/MapReduce_Rust
 * worker data path: map -> SipHash partition -> (shuffle) -> sort -> group/reduce -> mr-{r}.txt.
 *
 * Plain pointers and sizes only.  Every call returns MRG_OK (0) or a negative MRG_E* code and never
 * aborts across the ABI; mrg_last_error() gives a thread-local message for the last failure.
 * Device pointers ("d_") are HIP device allocations on the context's device; host pointers ("h_").
 *
 * Reference interfaces each entry point replaces (paths relative to the reference repo root):
 *   mrg_map        call_map_func(Box::new(wc::map), &contents)      src/mr/worker.rs:16-18, 147-150
 *                  + cal_hash_for_key / index = h % reduce_n        src/mr/worker.rs:111-115, 129
 *                  + write_key_value_to_file (partitioned output)   src/mr/worker.rs:117-140
 *                  wc::map                                          src/app/wc.rs:6-13
 *   mrg_reduce     read_file_to_mem_reduce + sort + group loop      src/mr/worker.rs:79-109, 157-193
 *                  call_reduce_func(Box::new(wc::reduce), ...)      src/mr/worker.rs:20-25, 174-178
 *                  wc::reduce                                       src/app/wc.rs:15-17
 *   mrg_run_job    the whole mrcoordinator + N x mrworker run       src/bin/mrworker.rs:43-149,
 *                  (static plan instead of coordinator.rs:137-215 task assignment), 1..8 GPUs
 *   mrg_job_shuffle the mr-{m}-{r}.txt hand-off between map and reduce workers through the shared
 *                  CWD (write_key_value_to_file worker.rs:117-140 -> read_file_to_mem_reduce
 *                  worker.rs:79-109), as one RCCL all-to-all over xGMI (owner of r = r % n_ranks)
 *   mrg_map_text   write_key_value_to_file, byte-exact mr-{m}-{r}.txt  src/mr/worker.rs:117-140
 *   mrg_reduce_text read_file_to_mem_reduce over mr-{m}-{r}.txt      src/mr/worker.rs:79-109, 157-193
 *   mrg_job_final  generate_output: cat mr-* | sort > final.txt     src/run.sh:16-20
 *   mrg_job_*      the same path with device-resident input, split at the shuffle so that a
 *                  multi-GPU host can exchange partitions between GPUs (RCCL all-to-all).
 */
#ifndef MRGPU_H
#define MRGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes ---- */
#define MRG_OK 0
#define MRG_EINVAL (-1)   /* bad argument / state (reference: assert! failures, worker.rs:130,143-160) */
#define MRG_EUTF8 (-2)    /* input is not UTF-8 (reference: read_to_string().unwrap() panics, worker.rs:75) */
#define MRG_EHIP (-3)     /* HIP runtime error */
#define MRG_ENOMEM (-4)   /* device or host allocation failed */
#define MRG_EIO (-5)      /* file open/read/write failed (reference: unwrap/`?` on fs ops, worker.rs:73,122,168) */
#define MRG_ECOMM (-6)    /* RCCL communicator error, or another rank of the job failed */

/* ---- apps (the reference selects wc at compile time, worker.rs:5,148,175) ---- */
#define MRG_APP_WC 0       /* src/app/wc.rs */
#define MRG_APP_INDEXER 1  /* build-defined (no indexer in the reference): word -> "n doc1,doc2,..." */

/* ---- flags ---- */
#define MRG_FLAG_NO_COMPAT_DROP_LAST 0x1u  /* default (flag clear): reproduce worker.rs:169-184, which never
                                              writes the last group of a partition.  Set: write it. */
#define MRG_FLAG_FINAL_TXT 0x2u  /* mrg_run_job: also write out_dir/final.txt (src/run.sh:16-20) */
#define MRG_FLAG_STREAM 0x4u   /* mrg_run_job only: map each GPU's files in batches while the next batch is read */
/* bits 8..15: truncate every internal (non-partition) hash to this many bits; 0 = full 64 bits.
   A test knob that forces hash collisions so the full-string tie-break paths are exercised. */
#define MRG_FLAG_DEBUG_HASH_BITS(n) (((uint32_t)(n) & 0xFFu) << 8)
/* bits 16..31, mrg_run_job only (word count; every other entry point ignores them): also write
   out_dir/top.txt, the k (1..65535) most frequent lines of final.txt, see mrg_job_topk. */
#define MRG_FLAG_TOP(k) (((uint32_t)(k) & 0xFFFFu) << 16)   /* mrg_run_job only: also write out_dir/top.txt */

/* Exchange record (mrg_job_export / mrg_job_import / mrg_parts): 24 bytes, little-endian.
 *   short key (len <= 16):
 *     u64 k0, k1   the key bytes, big-endian packed, zero padded (keys never contain NUL)
 *     u32 v        wc: occurrences (a key counted more than 0xFFFFFFFF times is sent as several records,
 *                  which the receiver sums); indexer: global document id
 *     u32 len      key length in bytes
 *   long key (len > 16):
 *     u64 heap     byte offset of the key bytes in the sender's heap segment
 *     u64 count    occurrences (wc) / 1 (indexer)
 *     u32 v        global document id (indexer), 0xFFFFFFFF (wc)
 *     u32 len      key length in bytes
 * The heap holds the bytes of keys longer than 16 bytes.  (Format 2; format 1 had 40-byte records.) */
#define MRG_XREC_BYTES 24

typedef struct mrg_ctx mrg_ctx;
typedef struct mrg_parts mrg_parts;
typedef struct mrg_vocab mrg_vocab;
#define MRG_ID_UNK 0xFFFFFFFFu   /* mrg_vocab_encode: the id of a word that is not in the vocabulary */

typedef struct {
    uint64_t input_bytes;      /* bytes mapped */
    uint64_t tokens;           /* tokens produced by the tokenizer */
    uint64_t long_tokens;      /* tokens longer than 16 bytes (slow path) */
    uint64_t map_records;      /* records leaving the map kernel (LDS-combine misses + flush) */
    uint64_t distinct_keys;    /* keys after aggregation (wc: words; indexer: (word, doc) pairs) */
    uint64_t output_bytes;     /* bytes of all mr-{r}.txt */
    double ms_map;             /* map kernel (tokenize + LDS combine), last call, HIP events */
    double ms_aggregate;       /* global aggregation + partition hash */
    double ms_sort;            /* radix sort */
    double ms_format;          /* output formatting */
    uint32_t map_launches;     /* map kernel launches in the last mrg_job_map */
    uint32_t agg_launches;     /* bucket-aggregation launches (> 1: its overflow list was regrown) */
    uint64_t overflow_keys;    /* records that took the exact HBM-table overflow path */
    double ms_exchange;        /* mrg_job_shuffle: the data send/recv group, HIP events on the ctx stream */
    uint64_t exchange_sent;    /* bytes this rank sent to peers (records + heap; its own slice excluded) */
    uint64_t exchange_recv;    /* bytes this rank received from peers */
    uint64_t map_spill;        /* map records that overflowed their tail region into a bucket's shared
                                  overflow list (last map launch) */
    uint64_t nonascii_tiles;   /* 1 KiB tiles that took the non-ASCII tokenizer (last map launch) */
    uint64_t tail_records_16;  /* wc: map records stored as 16-byte tail records (keys of 13..16 bytes; the
                                  others are 12-byte records); 0 for the indexer (all 24-byte records) */
    uint32_t spec_agg;         /* the aggregation queued behind the map: 0 none, 1 used, 2 dropped */
    uint32_t agg_path;         /* aggregation taken: 0 none, 1 bucket tables, 2 wide (sort-based) */
    uint32_t map_kind;         /* map kernel: 0 LDS combine + hash-bucketed tail records, 1 the wide map
                                  (near-unique keys: every key straight to its sort bucket) */
    uint32_t map_batches;      /* successful mrg_job_map_add calls of the job (0 after mrg_job_map / mrg_job_import);
                                  was `reserved`.  After mrg_job_map_add, input_bytes, tokens and long_tokens are
                                  totals over the job's batches, distinct_keys is the job's exact count so far,
                                  and the ms_*, launch and path fields describe the last batch */
} mrg_stats;

/* ABI history: 1 = round-1 layout; 2 = mrg_run_job's last argument is n_gpus (was a device index);
 * 3 = 24-byte exchange records (were 40), mrg_run_get_stats; 4 = mrg_stats gains nonascii_tiles,
 * tail_records_16, spec_agg, agg_path; 5 = mrg_stats gains map_kind, mrg_comm_count, mrg_pool_stats;
 * 6 = mrg_pool_alloc_stats.  mrg_version() names the ABI it implements.
 * (6, additive): mrg_job_topk, mrg_job_copy_topk, MRG_FLAG_TOP
 * (6, additive): mrg_job_map_add, MRG_FLAG_STREAM, mrg_run_get_stream_stats; mrg_stats.reserved is now
 * map_batches (same size and offset)
 * (6, additive): mrg_job_vocab, mrg_vocab_size, mrg_vocab_copy_text, mrg_vocab_free, mrg_vocab_encode,
 * MRG_ID_UNK
 * (6, additive): mrg_vocab_from_text, mrg_vocab_decode
 * (6, additive): mrg_vocab_term_counts
 * (6, additive): mrg_vocab_postings
 * (6, additive): mrg_vocab_search
 * (6, additive): mrg_vocab_stats_add, mrg_vocab_search_shard, mrg_search_merge, MRG_SEARCH_MAX_SHARDS
 * (6, additive): mrg_vocab_postings_merge
 * (6, additive): mrg_vocab_search_bool, mrg_vocab_search_bool_shard, MRG_Q_SHOULD, MRG_Q_MUST, MRG_Q_MUST_NOT */
#define MRG_ABI_VERSION 6

const char *mrg_last_error(void);
const char *mrg_version(void);

/* One context per thread and device.  Owns a HIP stream (or uses one set by mrg_set_stream) and all
 * device workspaces, which grow on demand and are reused across jobs. */
int mrg_open(int device, mrg_ctx **out);
int mrg_close(mrg_ctx *ctx);
/* Run every kernel of this context on `hip_stream` (a hipStream_t; NULL = the context's own). */
int mrg_set_stream(mrg_ctx *ctx, void *hip_stream);
int mrg_get_stats(mrg_ctx *ctx, mrg_stats *out);
/* Per-stage HIP-event timing (mrg_stats.ms_*); off by default (it adds events to the stream). */
int mrg_set_timing(mrg_ctx *ctx, int enable);

/* ---- device-resident job (bench, multi-GPU) ---- */

/* Start a job.  n_reduce = nReduce (worker.rs:129).  Clears previous job state. */
int mrg_job_begin(mrg_ctx *ctx, int app, uint32_t n_reduce, uint32_t flags);
/* Document names, indexed by global document id (indexer output; ignored by wc).  Every rank of a
 * multi-GPU job passes the full table.  Names must not contain ' ', ',' or '\n'.
 * Every document id the job's keys carry (from mrg_job_set_input, mrg_map or mrg_job_import) must be below
 * n_names: mrg_job_reduce and mrg_job_final return MRG_EINVAL for an id that has no name. */
int mrg_job_set_doc_names(mrg_ctx *ctx, const char *const *names, uint32_t n_names);
/* Input: documents laid out back to back in ONE device buffer d_bytes (16-byte aligned);
 * document i is d_bytes[h_doc_off[i] .. h_doc_off[i+1]) with global id h_doc_ids[i] (NULL: i).
 * The buffer is borrowed until the next mrg_job_begin.
 * Indexer: an id is not checked here (the names may be set later); an id at or above the n_names of
 * mrg_job_set_doc_names makes mrg_job_reduce and mrg_job_final return MRG_EINVAL. */
int mrg_job_set_input(mrg_ctx *ctx, const uint8_t *d_bytes, const uint64_t *h_doc_off, uint32_t n_docs,
                      const uint32_t *h_doc_ids);
/* Map: tokenize (wc.rs:6-13) + combine + SipHash partition (worker.rs:111-115).  Validates UTF-8. */
int mrg_job_map(mrg_ctx *ctx);
/* Map the input set by mrg_job_set_input and ADD its tokens to the job's keys.
 * mrg_job_map replaces the job's keys; this call adds to them.
 * After mrg_job_begin the caller may repeat { mrg_job_set_input, mrg_job_map_add } any number of times;
 * every consumer (export, shuffle, reduce, final, topk) then behaves as if one mrg_job_map had run over
 * all the batches' documents together, byte for byte.  Consumers may be called between batches and more
 * batches may follow.  A batch holds whole documents (a token across a cut would become two); indexer
 * batches pass global ids in h_doc_ids, and mrg_job_set_doc_names is given once with the full table.
 * Keys the job already holds (mrg_job_map, mrg_job_import) are added to; mrg_job_map and mrg_job_import
 * still replace everything.  All-or-nothing: when the map fails (MRG_EUTF8, MRG_ENOMEM) the job keeps
 * exactly the keys it had and stays usable.  The device no longer reads the batch's buffer once this
 * call returns: the caller may overwrite or free it then (mrg_job_map's contract is unchanged). */
int mrg_job_map_add(mrg_ctx *ctx);
/* Shuffle boundary.  Owner of partition r is r % n_owners.  Sizes first (host arrays of n_owners),
 * then pack into caller device buffers ordered by owner (records, then heap bytes). */
int mrg_job_export_sizes(mrg_ctx *ctx, uint32_t n_owners, uint64_t *h_rec_counts, uint64_t *h_heap_bytes);
int mrg_job_export(mrg_ctx *ctx, void *d_rec, void *d_heap);
/* Replace the job's keys by the aggregation of received exchange records: the concatenation of
 * n_segs senders' exports, sender i contributing h_seg_recs[i] records and h_seg_heap[i] heap bytes
 * (record heap offsets are relative to their sender's heap segment).  n_segs = 0: one segment. */
int mrg_job_import(mrg_ctx *ctx, const void *d_rec, uint64_t n_rec, const void *d_heap, uint64_t heap_bytes,
                   const uint64_t *h_seg_recs, const uint64_t *h_seg_heap, uint32_t n_segs);
/* Reduce: sort (byte order, worker.rs:162-164), group, reduce, format every owned partition.
 * *h_out_bytes = total bytes of the mr-{r}.txt contents (concatenated in r order). */
int mrg_job_reduce(mrg_ctx *ctx, uint64_t *h_out_bytes);
/* Device pointer to the output and the byte offset of each partition (h_part_off[n_reduce + 1]). */
int mrg_job_output(mrg_ctx *ctx, const uint8_t **d_out, uint64_t *h_part_off);
/* Copy the output to host memory (h_dst of at least *h_out_bytes). */
int mrg_job_copy_output(mrg_ctx *ctx, uint8_t *h_dst, uint64_t cap);
/* final.txt of src/run.sh:16-20 (generate_output: cat mr-* | sort > final.txt, with LC_ALL=C), built
 * on the device from the job's keys: every line of every mr-{r}.txt this context holds, sorted
 * bytewise (= by key: key bytes are all > ' ').  *d_out stays valid until the next job call. */
int mrg_job_final(mrg_ctx *ctx, const uint8_t **d_out, uint64_t *h_bytes);
int mrg_job_copy_final(mrg_ctx *ctx, uint8_t *h_dst, uint64_t cap);
/* The k most frequent words (word count only): the first min(k, lines) lines of what mrg_job_final
 * would produce now (so with the last group of every partition dropped unless
 * MRG_FLAG_NO_COMPAT_DROP_LAST), ordered by count descending, then key bytes ascending; each line
 * byte-identical to its final.txt line.  Selected on the device (a radix select over the counts: the
 * keys are not sorted).  Callable whenever mrg_job_final is, any number of times, with any k; it
 * leaves the job as it was.  *d_out stays valid until the next job call; *h_lines = lines written.
 * Any out pointer may be NULL.  k = 0 or no lines: zero bytes, MRG_OK. */
int mrg_job_topk(mrg_ctx *ctx, uint64_t k, const uint8_t **d_out, uint64_t *h_bytes, uint64_t *h_lines);
int mrg_job_copy_topk(mrg_ctx *ctx, uint8_t *h_dst, uint64_t cap);

/* ---- vocabulary: the most frequent words as ids 0..n-1, and text -> id sequences on the device ----
 * mrg_job_vocab freezes the job's most frequent words into a vocabulary object (word count only: the
 * indexer gets MRG_EINVAL).  Callable whenever mrg_job_topk is (between mrg_job_map_add batches and
 * after mrg_job_import too).  The word with id i is line i of what mrg_job_topk(ctx, max_words, ...)
 * would return now: count descending, then key bytes ascending, with the last group of every partition
 * dropped unless the job has MRG_FLAG_NO_COMPAT_DROP_LAST -- set that flag for a complete vocabulary.
 * The list is cut at the first word whose count is below min_count (0 and 1: no cut).  max_words = 0:
 * all words; more than 0xFFFFFFFE resulting words: MRG_EINVAL.  An empty vocabulary is valid.  The
 * job's keys stay as they were; like any job call it may invalidate d_out pointers of earlier topk /
 * final calls (and it replaces the lines mrg_job_copy_topk returns).  On failure *out is NULL and
 * nothing is leaked.
 * The vocabulary owns its device memory (the words' bytes are copied: nothing is borrowed from the
 * job, the input buffer or the context's pool), so it survives mrg_job_begin, later jobs and mrg_close
 * of the context that made it.  It is read-only after creation: any context on the same device may use
 * it, from several threads at once; a context on another device gets MRG_EINVAL.  It inherits
 * MRG_FLAG_DEBUG_HASH_BITS from its job.  mrg_vocab_free(NULL) is a no-op. */
int mrg_job_vocab(mrg_ctx *ctx, uint64_t max_words, uint64_t min_count, mrg_vocab **out);
/* Words in the vocabulary and bytes of its text.  Either pointer may be NULL. */
int mrg_vocab_size(const mrg_vocab *v, uint64_t *n_words, uint64_t *text_bytes);
/* The "word count\n" lines in id order, each byte-identical to the mrg_job_topk line the word came
 * from, to host memory.  cap below the text's bytes: MRG_EINVAL. */
int mrg_vocab_copy_text(const mrg_vocab *v, uint8_t *h_dst, uint64_t cap);
void mrg_vocab_free(mrg_vocab *v);
/* Text -> ids.  Input as for mrg_job_set_input: documents back to back in d_bytes (16-byte aligned),
 * document i = d_bytes[h_doc_off[i] .. h_doc_off[i+1]).  The tokens are exactly those of wc::map
 * (src/app/wc.rs:6-13), per document, in input order: a token is a maximal run of non-White_Space
 * codepoints, its key the token's \w codepoints; a token with an empty key produces nothing; a token
 * never crosses a document boundary.  d_ids[h_tok_off[i] .. h_tok_off[i+1]) receives document i's ids
 * (h_tok_off has n_docs + 1 entries); a word not in the vocabulary gets MRG_ID_UNK.  Identity is the
 * full key bytes, always (keys longer than 16 bytes are compared byte for byte).
 * d_ids = NULL: count only -- h_tok_off is filled, nothing is written to the device output.  Otherwise
 * cap_ids (in ids) < h_tok_off[n_docs] returns MRG_EINVAL with d_ids untouched.  Invalid UTF-8 returns
 * MRG_EUTF8 (mrg_last_error names the document and the byte offset, as for the map); d_ids is then
 * unspecified; the context, its job and the vocabulary stay usable.  The call needs no job and touches
 * no job state (it is legal between the batches of a streamed job).  It runs on the context's stream
 * with scratch from the context's pool (about 1/7 of the input's bytes), all returned before the call
 * ends; on return the ids are complete and the caller may free or overwrite the input. */
int mrg_vocab_encode(mrg_ctx *ctx, const mrg_vocab *v, const uint8_t *d_bytes, const uint64_t *h_doc_off,
                     uint32_t n_docs, uint32_t *d_ids, uint64_t cap_ids, uint64_t *h_tok_off);

/* A vocabulary from its text, on any device.  h_text is host memory holding `bytes` bytes of
 * "word count\n" lines: what mrg_vocab_copy_text returns, or the top.txt or final.txt of a word-count
 * mrg_run_job (so the whole ranking of a multi-GPU job, which no single context holds, becomes a
 * vocabulary this way).  The word on line i (0-based) gets id i; the lines need not be ordered by count
 * (a final.txt, in key order, gives ids in key order).  The result is an ordinary mrg_vocab on ctx's
 * device with the ownership and lifetime rules above: one device allocation of its own, it survives
 * mrg_job_begin and mrg_close, it is read-only and any context of that device may use it from several
 * threads.  mrg_vocab_copy_text of it returns h_text byte for byte; mrg_vocab_size returns (lines,
 * bytes).  The call needs no job and touches no job state; its scratch comes from the context's pool
 * and is all returned before it ends.  Of `flags` only the MRG_FLAG_DEBUG_HASH_BITS(n) bits are read
 * (the role the job's flags play for mrg_job_vocab); any other bit set: MRG_EINVAL.  bytes = 0 gives
 * the valid empty vocabulary (h_text may then be NULL).  More than 0xFFFFFFFE lines: MRG_EINVAL.
 * Validation -- MRG_EINVAL unless stated, mrg_last_error names the 0-based line ("line N"), *out is
 * NULL, nothing is leaked, the context and every other vocabulary stay usable:
 *   - the text is empty or ends in '\n';
 *   - every line is valid UTF-8 (else MRG_EUTF8, with the line named, as the map reports it): checked
 *     first, over the whole line, so a line that strict UTF-8 decoding rejects is MRG_EUTF8 whatever
 *     else is wrong with it;
 *   - every line is `word`, one ' ', then 1 to 20 ASCII digits (the count is not interpreted further):
 *     an empty line, a missing count or a second space is an error; the word is not empty;
 *   - every codepoint of the word is \w by the map's tables, i.e. the word is accepted exactly when
 *     wc::map over it produces that word as its single key (don't, a-dash-b and "a b" are rejected);
 *   - no word stands on two lines ("duplicate", naming a line whose word also stands on another one);
 *     words longer than 16 bytes are compared byte for byte, under MRG_FLAG_DEBUG_HASH_BITS too. */
int mrg_vocab_from_text(mrg_ctx *ctx, const uint8_t *h_text, uint64_t bytes, uint32_t flags, mrg_vocab **out);
/* Ids -> text, the inverse of mrg_vocab_encode with the same document layout: document i's ids are
 * d_ids[h_tok_off[i] .. h_tok_off[i+1]) (d_ids: device memory, 4-byte aligned; h_tok_off: n_docs + 1
 * non-decreasing entries).  Every id becomes its word's bytes followed by one separator byte: ' '
 * inside a document, '\n' after the document's last id; an empty document produces no bytes.
 * Document i's text is d_out[h_out_off[i] .. h_out_off[i+1]); h_out_off has n_docs + 1 entries and
 * h_out_off[0] = 0.  Encoding d_out with h_out_off as document offsets returns the original ids and
 * offsets, as long as the UNK bytes are \w-only and not a word of the vocabulary.
 * MRG_ID_UNK is written as the unk_len (0..255) bytes at h_unk (host memory, not validated); with
 * unk_len = 0 an MRG_ID_UNK is an error, as is any other id >= the vocabulary's words: MRG_EINVAL,
 * mrg_last_error names the index in d_ids of the first such id ("index N"), d_out is then unspecified,
 * the context and the vocabulary stay usable.
 * d_out = NULL: sizes only -- h_out_off is filled, nothing is written.  Otherwise cap (bytes) <
 * h_out_off[n_docs] returns MRG_EINVAL with d_out untouched.  n_docs = 0 or no ids: all-zero offsets,
 * MRG_OK.  A vocabulary of another device: MRG_EINVAL.
 * The call needs no job and touches no job state (it is legal between mrg_job_map_add batches).  It
 * runs on the context's stream with scratch from the context's pool (about 1/8 byte per id for the
 * boundary bitmap plus 8 bytes per 256 ids), all returned before the call ends; on return the text is
 * complete. */
int mrg_vocab_decode(mrg_ctx *ctx, const mrg_vocab *v, const uint32_t *d_ids, const uint64_t *h_tok_off,
                     uint32_t n_docs, const uint8_t *h_unk, uint32_t unk_len, uint8_t *d_out, uint64_t cap,
                     uint64_t *h_out_off);
/* Ids -> per-document term counts: the document-term matrix in CSR form.  The input layout is that of
 * mrg_vocab_decode: document i's ids are d_ids[h_tok_off[i] .. h_tok_off[i+1]) (d_ids: device memory,
 * 4-byte aligned; h_tok_off: n_docs + 1 non-decreasing entries, h_tok_off[0] may be greater than 0).
 * Row i is d_terms[h_row_off[i] .. h_row_off[i+1]): the distinct ids of document i other than MRG_ID_UNK,
 * in ascending order (a vocabulary of mrg_job_vocab is ranked, so that is most frequent in the vocabulary
 * first); d_counts at the same positions holds the occurrences of each id in that document.  h_row_off
 * has n_docs + 1 entries and h_row_off[0] = 0.  The output is fully determined by the input: no order
 * depends on scheduling.
 * MRG_ID_UNK never appears in a row.  h_unk may be NULL; otherwise h_unk[i] (n_docs entries) is the
 * number of MRG_ID_UNK in document i, so sum(counts of row i) + h_unk[i] = h_tok_off[i+1] - h_tok_off[i].
 * Any other id >= the vocabulary's words: MRG_EINVAL, mrg_last_error names the smallest index in d_ids
 * of such an id ("index N"), the outputs are then unspecified, the context and the vocabulary stay
 * usable.  An empty vocabulary is valid: every id must then be MRG_ID_UNK.
 * A document of more than 0xFFFFFFFF ids: MRG_EINVAL before any device work, so every count fits 32 bits.
 * d_terms = NULL and d_counts = NULL: sizes only -- h_row_off and h_unk are filled, nothing else is
 * written; exactly one of the two NULL: MRG_EINVAL.  Otherwise cap (entries of each buffer) <
 * h_row_off[n_docs] returns MRG_EINVAL with both buffers untouched.  cap >= the number of ids always
 * suffices, so a caller may skip the sizing call.  n_docs = 0 or no ids: all-zero offsets, MRG_OK.  A
 * vocabulary of another device: MRG_EINVAL.
 * The call needs no job and touches no job state (it is legal between mrg_job_map_add batches).  It
 * runs on the context's stream with scratch from the context's pool, all returned before the call ends,
 * on error exits too; on return the outputs are complete.  Scratch: 24 bytes per document, 4 bytes per
 * non-empty document, and for the documents of more than 4096 ids, which are processed in slices of at
 * most 2^25 ids together (a longer document alone), about 16.5 bytes per id of the largest slice. */
int mrg_vocab_term_counts(mrg_ctx *ctx, const mrg_vocab *v, const uint32_t *d_ids, const uint64_t *h_tok_off,
                          uint32_t n_docs, uint32_t *d_terms, uint32_t *d_counts, uint64_t cap,
                          uint64_t *h_row_off, uint64_t *h_unk);
/* Term counts -> the inverted index over ids: the transpose (CSC form) of the document-term matrix.  The
 * input is a CSR in the layout mrg_vocab_term_counts writes: row i is d_terms[h_row_off[i] .. h_row_off[i+1])
 * with d_counts at the same positions (device memory, 4-byte aligned; h_row_off: n_docs + 1 non-decreasing
 * entries).  h_row_off[0] may be greater than 0, so rows [a, b) of a bigger CSR are indexed by passing
 * h_row_off + a, n_docs = b - a and doc_base = a: the document of row i is doc_base + i.  E =
 * h_row_off[n_docs] - h_row_off[0] is the number of entries; only those entries are read.
 * d_post_off (device memory, 8-byte aligned) receives the vocabulary's words + 1 offsets, d_post_off[0] = 0
 * and d_post_off[words] = E.  The postings of word w are d_docs[d_post_off[w] .. d_post_off[w+1]) with the
 * term frequencies in d_tf at the same positions; the document frequency of w is d_post_off[w+1] -
 * d_post_off[w].  The call is a stable transpose: the postings of a word stand in the input order of its
 * entries, so its documents ascend; a term that stands twice in a row gives two postings of that document,
 * in entry order; nothing is required of the order inside a row; a count is copied as it is, 0 included.
 * The output is fully determined by the input: no order depends on scheduling, two calls give identical
 * bytes.
 * d_docs = NULL and d_tf = NULL: document frequencies only -- only d_post_off is written, d_counts is not
 * read and may be NULL.  d_tf = NULL: documents only, d_counts is not read.  d_tf without d_docs, or d_tf
 * without d_counts: MRG_EINVAL.  h_entries may be NULL; otherwise it receives E.
 * Checked before any device work, MRG_EINVAL with every output untouched: a NULL context, a vocabulary of
 * another device, offsets that are not non-decreasing, doc_base + n_docs > 2^32, E >= 2^32, d_post_off =
 * NULL, the NULL combinations above, and d_docs != NULL with cap (entries of d_docs and of d_tf) < E
 * ("too small").  Checked on the device: a term >= the vocabulary's words (MRG_ID_UNK included, which never
 * stands in a row) is MRG_EINVAL, mrg_last_error names the smallest index in d_terms of such a term
 * ("index N"), the outputs are then unspecified.  After every error the context and the vocabulary stay
 * usable.  An empty vocabulary is valid: E must then be 0 and d_post_off gets its one 0.  n_docs = 0 or
 * E = 0: all-zero offsets, MRG_OK.
 * The call needs no job and touches no job state (it is legal between mrg_job_map_add batches).  It runs
 * on the context's stream with scratch from the context's pool, all returned before the call ends, on
 * error exits too; on return the outputs are complete.  Scratch: nothing per word beyond the scan's 8
 * bytes per 2048 words (the frequencies are counted in d_post_off itself); for the postings 24.5 bytes
 * per entry (two 12-byte records and the sort's tile counts) and 8 bytes per row. */
int mrg_vocab_postings(mrg_ctx *ctx, const mrg_vocab *v, const uint32_t *d_terms, const uint32_t *d_counts,
                       const uint64_t *h_row_off, uint32_t n_docs, uint32_t doc_base, uint64_t *d_post_off,
                       uint32_t *d_docs, uint32_t *d_tf, uint64_t cap, uint64_t *h_entries);
/* (6, additive): mrg_vocab_search.  The inverted index + a batch of queries -> the k best documents of every
 * query by BM25, on the device.  d_post_off (words + 1), d_docs and d_tf are what mrg_vocab_postings wrote for
 * this vocabulary, n_entries its E.  The collection is the documents doc_base .. doc_base + n_docs - 1;
 * d_doc_len[i] (device, n_docs uint32) is the length in ids of document doc_base + i, MRG_ID_UNK ids included
 * (h_tok_off[i+1] - h_tok_off[i] of mrg_vocab_encode).  The queries are laid out like the documents of
 * mrg_vocab_decode: query q is d_q_ids[h_q_off[q] .. h_q_off[q+1]) -- device ids, host offsets, h_q_off[0] may
 * be greater than 0 -- which is what mrg_vocab_encode of the query texts returns.  At most 2^20 query ids in one
 * call (the library copies them to the host).
 * The score is BM25 with the always-positive idf, over the one index passed:
 *   N = n_docs;  avgdl = (sum of d_doc_len) / N      (summed exactly, divided in double, rounded to float)
 *   df(t) = d_post_off[t+1] - d_post_off[t]
 *   idf(t) = ln(1 + (N - df + 0.5) / (df + 0.5))     (in double, rounded to float)
 *   w(t,d) = idf(t) * tf*(k1+1) / (tf + k1*(1 - b + b*dl(d)/avgdl))      (float32)
 *   score(q,d) = the sum over the positions j of q, in order, of w(q[j], d)
 * A term that stands m times in a query counts m times; an MRG_ID_UNK position and a term with no postings
 * count nothing.  A document is a hit of q when its score is > 0.
 * h_top_n[q] = min(k, hits of q); row q of the output is d_top_docs[q*k .. q*k + h_top_n[q]) with d_top_scores
 * at the same positions, by score descending, then document ascending; the documents carry doc_base.  The
 * entries of a row from h_top_n[q] on are not written.  The selection at the k-th place is exact: every
 * document above the k-th score is returned, and of those with exactly the k-th score the smallest documents.
 * The output is fully determined by the input: two calls give identical bytes, whatever the scheduling and
 * however the call cuts the queries into chunks (MRG_SEARCH_ACC_BYTES, an environment variable read per call,
 * default 256 MiB: the bytes of dense score rows, n_docs floats per query, that are worked on together; a
 * query whose one row does not fit is taken alone).
 * Checked before any device work, MRG_EINVAL with every output untouched: a NULL context or vocabulary, a
 * vocabulary of another device, NULL d_post_off, h_q_off, d_top_docs, d_top_scores or h_top_n, NULL d_docs,
 * d_tf or d_doc_len with n_entries > 0, misaligned pointers (4 bytes; d_post_off 8), offsets that are not
 * non-decreasing, doc_base + n_docs > 2^32, n_entries >= 2^32, k outside 1..MRG_SEARCH_MAX_K, k1 outside
 * [0, 1000], b outside [0, 1], either one NaN, more than 2^20 query ids.  Checked against the device's data,
 * MRG_EINVAL with the outputs unspecified: a query id >= the vocabulary's words other than MRG_ID_UNK
 * (mrg_last_error names the smallest index in d_q_ids, "index N"); for the words the queries name,
 * d_post_off[t] <= d_post_off[t+1] <= n_entries; every visited posting's document lies in the collection and
 * the documents of a visited word ascend strictly, as mrg_vocab_term_counts -> mrg_vocab_postings produces
 * them (mrg_last_error names the smallest offending position in d_docs, "posting N").  These checks are part
 * of the kernel: the call never writes outside its accumulators.  After every error the context and the
 * vocabulary stay usable.  n_queries = 0, n_docs = 0, n_entries = 0, an empty vocabulary (every id must then
 * be MRG_ID_UNK) or all-empty queries: h_top_n all 0, MRG_OK.
 * The call needs no job and touches no job state.  It runs on the context's stream with scratch from the
 * context's pool, all returned before the call ends, on error exits too; on return the outputs are complete.
 * Scratch: per query of a chunk 4 bytes per document (the row), 8 k bytes of candidates and 1 KiB; 20 bytes
 * per 4096 postings visited; 16 bytes per query id. */
#define MRG_SEARCH_MAX_K 1024u
int mrg_vocab_search(mrg_ctx *ctx, const mrg_vocab *v, const uint64_t *d_post_off, const uint32_t *d_docs,
                     const uint32_t *d_tf, uint64_t n_entries, const uint32_t *d_doc_len, uint32_t n_docs,
                     uint32_t doc_base, const uint32_t *d_q_ids, const uint64_t *h_q_off, uint32_t n_queries,
                     float k1, float b, uint32_t k, uint32_t *d_top_docs, float *d_top_scores, uint32_t *h_top_n);

/* ---- search over a sharded index (6, additive) ----
 * An index built batch by batch (mrg_vocab_postings with doc_base), or on the GPUs of one job, is a set of shards:
 * each holds all the postings of its own documents, and the shards partition the collection.  Three calls search
 * them as one: mrg_vocab_stats_add gathers the collection's statistics, mrg_vocab_search_shard scores one shard
 * with them, mrg_search_merge merges the shards' rows.  The result is, byte for byte, that of mrg_vocab_search
 * over the index in one piece: a cell of a score row receives the same float additions in the same query order
 * from the same idf and avgdl floats, a shard's selection is exact under the total order (score descending,
 * document ascending), so the collection's top-k is a subset of the union of the shards' top-k.
 *
 * mrg_vocab_stats_add: one shard's part of the statistics.  d_df (device memory, the vocabulary's words uint64,
 * 8-byte aligned, zeroed by the caller before the first shard) receives d_df[w] += d_post_off[w+1] -
 * d_post_off[w]; h_coll (two host uint64 that the caller starts at 0) receives h_coll[0] += n_docs and
 * h_coll[1] += the sum of d_doc_len (n_docs uint32 on the device, summed there in integers).  Integers only: the
 * result does not depend on the order of the shards.  d_df is a plain array on purpose: the shards of a multi-GPU
 * job add their arrays with whatever all-reduce the host has, or through host memory.
 * Checked before any device work, MRG_EINVAL with nothing written: a NULL context, vocabulary, d_post_off, d_df
 * or h_coll, NULL d_doc_len with n_docs > 0, misaligned pointers (8 bytes; d_doc_len 4), a vocabulary of another
 * device.  Checked on the device: d_post_off[w+1] < d_post_off[w] is MRG_EINVAL, mrg_last_error names the
 * smallest such word ("word N"), h_coll is untouched and d_df then unspecified.  An empty vocabulary or n_docs =
 * 0 is valid.  Needs no job; runs on the context's stream with 16 bytes of pool scratch, returned on every exit. */
int mrg_vocab_stats_add(mrg_ctx *ctx, const mrg_vocab *v, const uint64_t *d_post_off, const uint32_t *d_doc_len,
                        uint32_t n_docs, uint64_t *d_df, uint64_t *h_coll);
/* mrg_vocab_search_shard: mrg_vocab_search over one shard, scored with the collection's statistics.  Everything
 * is as for mrg_vocab_search -- layout, validation, chunking by MRG_SEARCH_ACC_BYTES, output rows, the exact
 * k-th place, the "index N" and "posting N" errors, scratch (8 more bytes per query id) -- except
 *   N = coll_docs;  avgdl = coll_sum_len / coll_docs    (in double, rounded to float; 1 when every length is 0)
 *   df(t) = d_df[t]
 * with d_df, coll_docs = h_coll[0] and coll_sum_len = h_coll[1] as mrg_vocab_stats_add left them after the last
 * shard.  The shard's own d_post_off still decides which postings are visited: a word with no postings in this
 * shard counts nothing, whatever its d_df.  The documents of the rows carry the shard's doc_base.
 * Refused in addition, MRG_EINVAL: before any device work a NULL or misaligned (8 bytes) d_df when the vocabulary
 * has words, coll_docs < n_docs, coll_docs > 2^32; from the gathered values, before any accumulate launch, for a
 * word the queries name that has postings in this shard: d_df[t] below the shard's own document frequency or
 * above coll_docs ("d_df of word N").
 * With the statistics of this one index the output is byte-identical to mrg_vocab_search. */
int mrg_vocab_search_shard(mrg_ctx *ctx, const mrg_vocab *v, const uint64_t *d_post_off, const uint32_t *d_docs,
                           const uint32_t *d_tf, uint64_t n_entries, const uint32_t *d_doc_len, uint32_t n_docs,
                           uint32_t doc_base, const uint64_t *d_df, uint64_t coll_docs, uint64_t coll_sum_len,
                           const uint32_t *d_q_ids, const uint64_t *h_q_off, uint32_t n_queries, float k1, float b,
                           uint32_t k, uint32_t *d_top_docs, float *d_top_scores, uint32_t *h_top_n);
/* mrg_search_merge: the result rows of n_shards searches over the same n_queries queries -> the collection's
 * rows, on the device.  Row [s, q] of the input is d_in_docs[(s * n_queries + q) * k_in ..] with d_in_scores at
 * the same positions and h_in_top_n[s * n_queries + q] entries: a shard's search with k = k_in writes its rows
 * straight into its slice of the buffers and its counts into its slice of h_in_top_n; rows of other devices, at
 * most 8 KiB per query, are the caller's to copy.  The output is laid out like the search's: row q of k_out
 * slots, h_top_n[q] = min(k_out, the sum over s of the in-counts), by score descending, then document ascending,
 * then shard ascending -- the last key makes the order total should a caller pass shards that overlap, which is
 * neither checked nor an error.  The entries of a row from h_top_n[q] on are not written.  Two calls give
 * identical bytes.
 * When the shards partition the documents and every shard was searched with k >= k_out (documented, not
 * checked), the merged rows equal those of mrg_vocab_search over the whole collection with k = k_out, byte for
 * byte.  The output of a merge is a valid input row, so more than MRG_SEARCH_MAX_SHARDS shards merge in stages.
 * Checked before any device work, MRG_EINVAL with every output untouched: NULL pointers, misaligned device
 * pointers (4 bytes), n_shards outside 1..MRG_SEARCH_MAX_SHARDS, k_in or k_out outside 1..MRG_SEARCH_MAX_K, an
 * in-count above k_in, n_shards * n_queries * k_in >= 2^32.  Checked in the kernel, MRG_EINVAL with the outputs
 * unspecified: every used entry has a score that is positive and no NaN, and stands strictly after its
 * predecessor in its row -- a lower score, or an equal score and a higher document (mrg_last_error names the
 * smallest offending flat index in d_in_docs, "entry N").  The call never writes outside the output rows.
 * n_queries = 0 or all counts 0: h_top_n all 0, MRG_OK.
 * The call needs no job and touches no job state.  It runs on the context's stream with scratch from the
 * context's pool (4 bytes per input row), returned before the call ends, on error exits too; on return the
 * outputs are complete. */
#define MRG_SEARCH_MAX_SHARDS 64u
int mrg_search_merge(mrg_ctx *ctx, uint32_t n_shards, uint32_t n_queries, uint32_t k_in, const uint32_t *d_in_docs,
                     const float *d_in_scores, const uint32_t *h_in_top_n, uint32_t k_out, uint32_t *d_top_docs,
                     float *d_top_scores, uint32_t *h_top_n);

/* ---- Boolean queries (6, additive) ----
 * mrg_vocab_search_bool, mrg_vocab_search_bool_shard: mrg_vocab_search and mrg_vocab_search_shard with a role for
 * every query position.  h_q_role (host memory) is indexed like d_q_ids: h_q_role[j] is the role of d_q_ids[j]
 * for j in h_q_off[0] .. h_q_off[n_queries] - 1, the entries below h_q_off[0] are not read; NULL means every
 * position is MRG_Q_SHOULD.  Everything not named here is as for the plain call -- layout, validation, chunking
 * by MRG_SEARCH_ACC_BYTES, the "index N" and "posting N" errors, the d_df checks of the shard call (for positions
 * of every role), the output rows, "the entries from h_top_n[q] on are not written", two calls giving identical
 * bytes.
 *   score(q,d) = the sum over the positions j of q whose role is SHOULD or MUST, in order, of w(q[j], d)
 * -- the same float32 additions in the same order that mrg_vocab_search performs for q with its MUST_NOT
 * positions deleted, so for a document that passes the filter the score is that call's score, bit for bit.
 * A document stands in the postings of a word when the index passed holds a posting of it for that word,
 * whatever the posting's tf: a tf of 0 satisfies MUST, triggers MUST_NOT, and adds 0 to the score.
 * d is a hit of q when d stands in the postings of the word of every MUST position, in the postings of the word
 * of no MUST_NOT position, and score(q,d) > 0.  Hence:
 *   a word that stands m times as MUST is required once and scores m times;
 *   a MUST position that is MRG_ID_UNK, or a word with no postings in this index, gives the query no hits (in
 *     a shard call: no hits in this shard), and none of the query's postings are visited then;
 *   a MUST_NOT position that is MRG_ID_UNK, or a word with no postings, excludes nothing;
 *   the same word as MUST and MUST_NOT gives no hits; the same word as SHOULD and MUST_NOT excludes its
 *     documents; where a MUST_NOT position stands in its query makes no difference;
 *   a query of MUST_NOT positions only has no hits: its score is 0.
 * h_top_n[q] = min(k, hits of q), and the selection at the k-th place is exact among the hits (score descending,
 * then document ascending).  With h_q_role = NULL, or every role MRG_Q_SHOULD, both calls run the plain search
 * and write byte for byte what mrg_vocab_search / mrg_vocab_search_shard write.
 * Shards that partition the documents, searched with mrg_vocab_search_bool_shard with k = k_in >= k_out and merged
 * with mrg_search_merge, give the rows of mrg_vocab_search_bool over the index in one piece with k = k_out, byte
 * for byte: a document lives in one shard, which holds all its postings and filters it alone.
 * Refused in addition, checked before any device work, MRG_EINVAL with every output untouched: a role above 2
 * (mrg_last_error names the smallest index, "role at index N").  The postings of MUST_NOT words are visited and
 * checked like the others ("posting N"), except their d_tf, which is not read.  The call never writes outside its
 * rows.  After every error the context and the vocabulary stay usable, and all pool scratch is returned.
 * Scratch: as for the plain call when every role is SHOULD.  Otherwise 4 more bytes per document and query of
 * a chunk (the match state: the distinct MUST words that hold the document, the top bit once a MUST_NOT word
 * does), so a chunk holds MRG_SEARCH_ACC_BYTES / (8 n_docs) queries, and 8 bytes per query that has a MUST or
 * MUST_NOT position. */
#define MRG_Q_SHOULD 0u    /* scores; not required (every position of mrg_vocab_search is this) */
#define MRG_Q_MUST 1u      /* scores; a hit stands in this word's postings */
#define MRG_Q_MUST_NOT 2u  /* scores nothing; a hit does not stand in this word's postings */
int mrg_vocab_search_bool(mrg_ctx *ctx, const mrg_vocab *v, const uint64_t *d_post_off, const uint32_t *d_docs,
                          const uint32_t *d_tf, uint64_t n_entries, const uint32_t *d_doc_len, uint32_t n_docs,
                          uint32_t doc_base, const uint32_t *d_q_ids, const uint8_t *h_q_role, const uint64_t *h_q_off,
                          uint32_t n_queries, float k1, float b, uint32_t k, uint32_t *d_top_docs, float *d_top_scores,
                          uint32_t *h_top_n);
int mrg_vocab_search_bool_shard(mrg_ctx *ctx, const mrg_vocab *v, const uint64_t *d_post_off, const uint32_t *d_docs,
                                const uint32_t *d_tf, uint64_t n_entries, const uint32_t *d_doc_len, uint32_t n_docs,
                                uint32_t doc_base, const uint64_t *d_df, uint64_t coll_docs, uint64_t coll_sum_len,
                                const uint32_t *d_q_ids, const uint8_t *h_q_role, const uint64_t *h_q_off,
                                uint32_t n_queries, float k1, float b, uint32_t k, uint32_t *d_top_docs,
                                float *d_top_scores, uint32_t *h_top_n);

/* (6, additive): mrg_vocab_postings_merge.  The indexes of the shards of one collection -> one index, on the
 * device; the merged index is searched with the plain mrg_vocab_search.  Shard s is what mrg_vocab_postings wrote
 * for this vocabulary: h_post_off[s] (device memory, words + 1 offsets), h_docs[s] and h_tf[s] (device memory, the
 * documents carrying their doc_base, the term frequencies) and h_entries[s], its E.  The three tables are host
 * arrays of n_shards device pointers.  The shards hold ascending document ranges in the order passed.
 * d_post_off (device memory, 8-byte aligned, words + 1) receives d_post_off[w] = the sum over the shards of
 * their offset of w: d_post_off[0] = 0 and d_post_off[words] = the sum of h_entries.  The postings of word w in
 * d_docs are those of shard 0, then shard 1, ..., each shard's in its own order, with d_tf at the same positions.
 * h_total may be NULL; otherwise it receives the sum of h_entries.  When the shards are consecutive row ranges
 * of one CSR, in order, the three outputs equal those of mrg_vocab_postings over the whole CSR byte for byte,
 * and are valid input of mrg_vocab_search with d_doc_len the caller's concatenation and doc_base the first
 * shard's.  A merged index is a valid shard, so more than MRG_SEARCH_MAX_SHARDS shards merge in stages of
 * adjacent shards.  The output is fully determined by the input: two calls give identical bytes; no atomic
 * writes an offset or a posting.
 * d_docs = NULL and d_tf = NULL: only the summed offsets are written, h_docs and h_tf may be NULL and no posting
 * is read.  d_tf = NULL: documents only, h_tf may be NULL.  d_tf with h_tf = NULL or with d_docs = NULL:
 * MRG_EINVAL.  A shard with 0 entries may have NULL document and term-frequency pointers.
 * Refused before any device work, MRG_EINVAL with every output untouched: a NULL context, vocabulary,
 * h_post_off, h_entries or d_post_off; a NULL h_post_off[s]; a vocabulary of another device; n_shards outside
 * 1..MRG_SEARCH_MAX_SHARDS; misaligned pointers (4 bytes; offsets 8); a sum of h_entries >= 2^32; d_docs != NULL
 * with cap (entries of d_docs and of d_tf) below that sum ("too small"); the NULL combinations above; entries in
 * an empty vocabulary; an output range (d_post_off over words + 1 offsets, d_docs and d_tf over the sum of
 * h_entries) that overlaps an input range of any shard.
 * Checked on the device, MRG_EINVAL with the outputs unspecified; mrg_last_error names "shard S word N", the
 * smallest word and for it the smallest shard.  The offsets of a shard: the first is 0, none is below the one
 * before it (N: the word whose end is below its start), the last is h_entries[s] (N: the last word); these are
 * checked before any posting is read or written, so the copy never leaves a shard's arrays or the sum of
 * h_entries entries of the output.  The seams, when documents are merged: for a word, the last document of a
 * non-empty shard list is strictly below the first document of the next non-empty one (S: the later shard), which
 * makes the merged word ascend strictly, as mrg_vocab_search requires.  The order inside a shard's list is not
 * checked here: the search checks what it visits.  After every error the context and the vocabulary stay usable.
 * An empty vocabulary (every h_entries[s] must be 0) or all shards empty: all-zero offsets, MRG_OK.
 * The call needs no job and touches no job state.  It runs on the context's stream with scratch from the
 * context's pool, all returned before the call ends, on error exits too; on return the outputs are complete.
 * Scratch: 40 bytes per shard and the scan's 8 bytes per 2048 words; when documents are merged, 4 bytes per
 * (shard, word): the place of every list in the output.  Nothing per entry. */
int mrg_vocab_postings_merge(mrg_ctx *ctx, const mrg_vocab *v, uint32_t n_shards, const uint64_t *const *h_post_off,
                             const uint32_t *const *h_docs, const uint32_t *const *h_tf, const uint64_t *h_entries,
                             uint64_t *d_post_off, uint32_t *d_docs, uint32_t *d_tf, uint64_t cap,
                             uint64_t *h_total);

/* ---- multi-GPU: one rank per GPU, the shuffle as an RCCL all-to-all over xGMI ----
 * The reference moves map output to the reduce workers through mr-{m}-{r}.txt files in a shared
 * directory (worker.rs:117-140 -> :79-109) and hands out tasks on demand (coordinator.rs:137-215).
 * Here the plan is static: rank g maps its input shard, partition r is reduced by rank r % n_ranks,
 * and the hand-off is one exchange of combined per-key records. */
#define MRG_COMM_ID_BYTES 128
typedef struct mrg_comm mrg_comm;
/* A fresh communicator id (an RCCL unique id): made by one rank, given to every rank out of band. */
int mrg_comm_get_id(uint8_t id[MRG_COMM_ID_BYTES]);
/* Join the communicator as `rank` of n_ranks, on ctx's device.  Collective over the n_ranks callers
 * (they must call it concurrently: separate processes, or one thread per GPU). */
int mrg_comm_init(mrg_ctx *ctx, const uint8_t id[MRG_COMM_ID_BYTES], int n_ranks, int rank, mrg_comm **out);
int mrg_comm_destroy(mrg_comm *comm);
/* The exchange step, collective over the communicator, after mrg_job_map on every rank: the job's
 * keys are packed by owner (r % n_ranks), the per-owner counts go through an all-to-all, the records
 * and long-key heap bytes through grouped send/recv on the ctx stream, and the received records
 * replace the job's keys (mrg_job_import).  Then mrg_job_reduce formats the partitions this rank
 * owns (the others come out empty).  Every rank must reach this call: a rank whose map failed must
 * still tell the others (the host's concern; mrg_run_job does it). */
int mrg_job_shuffle(mrg_ctx *ctx, mrg_comm *comm);
/* Ranks of the communicator as RCCL counts them (ncclCommCount): the bench reports it beside n_gpus. */
int mrg_comm_count(const mrg_comm *comm, int *n_ranks);

/* ---- diagnostics ---- */
/* The context's device buffer pool: blocks handed out and not yet returned (between calls this is
 * the job state the context keeps), and all bytes it holds (handed out + cached).  Either may be NULL. */
int mrg_pool_stats(mrg_ctx *ctx, uint64_t *outstanding, uint64_t *held_bytes);
/* Device allocations the pool has made since mrg_open (cumulative): hipMalloc calls, their bytes and
 * the host milliseconds spent inside them.  A fresh context's first job pays these; later jobs reuse
 * cached blocks.  Either pointer may be NULL.  (ABI 6.) */
int mrg_pool_alloc_stats(mrg_ctx *ctx, uint64_t *n_allocs, uint64_t *alloc_bytes, double *alloc_ms);

/* ---- plugin-surface equivalents, host buffers (one map task / one reduce task) ---- */

/* One map task over one input file's bytes: wc.rs:6-13 + worker.rs:117-140, combined per
 * partition.  doc = the document name (indexer value); doc_id its global id. */
int mrg_map(mrg_ctx *ctx, int app, const uint8_t *h_bytes, size_t n, const char *doc, uint32_t doc_id,
            uint32_t n_reduce, uint32_t flags, mrg_parts **out);
/* Records of partition r of a map output (exchange-record format above). */
int mrg_parts_get(const mrg_parts *parts, uint32_t r, const uint8_t **h_rec, uint64_t *n_rec,
                  const uint8_t **h_heap, uint64_t *heap_bytes);
void mrg_parts_free(mrg_parts *parts);
/* One reduce task: partition r of k map outputs -> exact bytes of mr-{r}.txt (worker.rs:157-193).
 * For the indexer, doc_names[id] names global document id (n_docs entries); MRG_EINVAL when a record of
 * the partition carries an id (mrg_map's doc_id) at or above n_docs. */
int mrg_reduce(mrg_ctx *ctx, int app, uint32_t r, const mrg_parts *const *in, size_t k, uint32_t n_reduce,
               uint32_t flags, const char *const *doc_names, uint32_t n_docs, uint8_t **h_out, size_t *h_out_len);

/* ---- the reference's text intermediates, byte for byte (wc) ---- */

/* One map task writing mr-{m}-{r}.txt exactly as Worker::write_key_value_to_file does
 * (src/mr/worker.rs:117-140): "{key} 1\n" for every token of wc::map (src/app/wc.rs:6-13) in input
 * order, into file r = SipHash-1-3(key) % n_reduce (worker.rs:111-115, 129).  *h_out receives the
 * n_reduce files' bytes concatenated (free with mrg_free); h_part_off[n_reduce + 1] their offsets. */
int mrg_map_text(mrg_ctx *ctx, const uint8_t *h_bytes, size_t n, uint32_t n_reduce, uint8_t **h_out,
                 uint64_t *h_part_off);
/* One reduce task over k intermediate files' contents (Worker::read_file_to_mem_reduce + reduce,
 * worker.rs:79-109, 157-193): UTF-8 checked (MRG_EUTF8), every non-empty line must be exactly
 * "key value" (MRG_EINVAL, the reference's assert!), values counted per key (wc.rs:15-17), keys in
 * byte order, the last group dropped unless MRG_FLAG_NO_COMPAT_DROP_LAST.  Returns mr-{r}.txt. */
int mrg_reduce_text(mrg_ctx *ctx, const uint8_t *const *h_files, const uint64_t *h_sizes, size_t k, uint32_t flags,
                    uint8_t **h_out, size_t *h_out_len);

/* The whole job (mrcoordinator + workers, mrworker.rs:43-149) on GPUs 0 .. n_gpus-1, one host thread
 * per GPU: GPU g reads and maps files m with m % n_gpus == g (the coordinator's map task ids,
 * coordinator.rs:137-176), the shuffle is mrg_job_shuffle, GPU g reduces and writes out_dir/mr-{r}.txt
 * for r % n_gpus == g (the reduce task ids, coordinator.rs:178-215).  With MRG_FLAG_FINAL_TXT also
 * out_dir/final.txt: each GPU sorts the lines it holds, the host merges the n_gpus sorted runs.
 * With MRG_FLAG_TOP(k) (word count only: MRG_EINVAL for the indexer, before any work) also
 * out_dir/top.txt: each GPU selects the k most frequent lines among the keys it owns
 * (mrg_job_topk), the host merges the n_gpus runs by (count descending, key ascending) and keeps k.
 * Indexer document names are the file paths as given (the reference opens "data/gut-{m}.txt").
 * Files are read by several host threads per GPU through pinned staging, overlapped with the copies
 * to the device.  Every phase runs on all GPUs and is joined before the next, and the exchange agrees
 * on every rank's status before each transfer: a failure on any GPU fails the call, never hangs it.
 * With MRG_FLAG_STREAM each GPU's files (in order) are cut into batches -- maximal runs of consecutive
 * files of at most MRG_STREAM_BATCH_BYTES (env; default 4 GiB) together, a larger file alone -- and
 * batch i is mapped (mrg_job_map_add) while a helper thread reads batch i + 1 into the other of two
 * device buffers: the input footprint is two batches instead of the whole input.  The output files are
 * byte-identical with and without the flag.
 * (ABI 2 changed the last argument from a device index to n_gpus.) */
int mrg_run_job(const char *const *files, size_t n_files, uint32_t n_reduce, int app, const char *out_dir,
                uint32_t flags, int n_gpus);

/* Wall-clock phases of the last mrg_run_job on the calling thread (host clock, milliseconds). */
typedef struct {
    double ms_total;        /* the whole call */
    double ms_open;         /* contexts + communicators */
    double ms_read;         /* input files -> device (read + H2D, overlapped; slowest GPU); MRG_FLAG_STREAM:
                               the time the GPU's thread waited for reads */
    double ms_map;          /* map + aggregation after the read (slowest GPU); MRG_FLAG_STREAM: the phase's
                               wall time minus ms_read */
    double ms_shuffle;      /* the exchange (0 without a communicator) */
    double ms_reduce;       /* sort + format + D2H of the output (+ final.txt) */
    double ms_write;        /* mr-{r}.txt (+ final.txt) files */
    uint64_t input_bytes;
    uint64_t output_bytes;  /* bytes of all mr-{r}.txt */
    int n_gpus;
    double ms_map_alloc;    /* of ms_map: host time inside the fresh contexts' device allocations (slowest
                               GPU; every mrg_run_job opens fresh contexts, ABI 6) */
    double ms_map_kernel;       /* of ms_map: the map kernel (HIP events, slowest GPU; ABI 6) */
    double ms_aggregate_kernel; /* of ms_map: the aggregation after it (HIP events, slowest GPU; ABI 6) */
} mrg_run_stats;
int mrg_run_get_stats(mrg_run_stats *out);
/* The last mrg_run_job of this thread: batches mapped on the GPU that mapped the most (0 without
 * MRG_FLAG_STREAM) and the largest GPU's bytes of device input buffers (unstreamed: its whole input).
 * Either may be NULL. */
int mrg_run_get_stream_stats(uint32_t *batches, uint64_t *peak_input_bytes);

/* Free host memory returned by the library (mrg_reduce / mrg_map_text / mrg_reduce_text output). */
void mrg_free(void *p);

/* ---- synthetic inputs for the benchmark (not on the data path) ---- */

/* Zipf(s) text over a vocabulary of `vocab` distinct lowercase words (BASELINE config C3/C4),
 * written to d_dst[0 .. n_bytes).  Deterministic in (seed, file_index); see DESIGN.md. */
int mrg_gen_zipf(mrg_ctx *ctx, uint8_t *d_dst, uint64_t n_bytes, uint64_t seed, uint64_t file_index,
                 uint32_t vocab, double s);
/* The same Zipf text in a given style: MRG_TEXT_ASCII (= mrg_gen_zipf) or MRG_TEXT_GUTENBERG (the
 * reference corpus's kind of Unicode: U+2019 apostrophes, U+201C/U+201D quotes, U+2014 dashes joining
 * words, Latin-1 letters; about one non-ASCII codepoint per 150 bytes). */
#define MRG_TEXT_ASCII 0
#define MRG_TEXT_GUTENBERG 1
int mrg_gen_text(mrg_ctx *ctx, uint8_t *d_dst, uint64_t n_bytes, uint64_t seed, uint64_t file_index,
                 uint32_t vocab, double s, uint32_t style);
/* Near-unique 12-character keys (BASELINE config C5): token i of file f, 1% repeats. */
int mrg_gen_unique(mrg_ctx *ctx, uint8_t *d_dst, uint64_t n_bytes, uint64_t seed, uint64_t file_index);

#ifdef __cplusplus
}
#endif
#endif /* MRGPU_H */
