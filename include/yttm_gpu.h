/* yttm_gpu.h -- inner C ABI: the individual HIP kernel stages behind yttm_mi355x.h.
 *
 * A host (the reference's C++ trainer, or the parity tests) can drive the stages one by one; every stage cites the
 * reference code it replaces.  All functions return 0 on success; the message of the last failure is available from
 * yttm_gpu_last_error().  Opaque handle; the caller owns host buffers, the library owns device buffers; one host
 * thread per context, the stream is internal.
 */
#ifndef YTTM_GPU_H
#define YTTM_GPU_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct yttm_ctx yttm_ctx;

int yttm_gpu_ctx_create(int device, yttm_ctx **out);
void yttm_gpu_ctx_destroy(yttm_ctx *ctx);
const char *yttm_gpu_last_error(void);

/* Finished trainings keep their device buffers in a pool for the next call (hipMalloc/hipFree of ~10 GB cost several ms and
 * synchronise the device).  This returns the cached buffers to the driver.  YTTM_NO_POOL=1 disables the pool.  (No reference
 * counterpart: bpe.cpp allocates with new/std containers.) */
void yttm_release_device_memory(void);
/* debug: the pool's state -- [0] bytes handed out and not yet returned, [1] bytes cached for reuse, [2] the high-water mark of [0] since the
 * last context was made, [3] allocations asked of the pool since then (YTTM_TEST_ALLOC_FAIL=N makes the N-th of them fail).  (No reference
 * counterpart.) */
void yttm_gpu_pool_stats(uint64_t out[4]);

/* Every YTTM_* environment hook of the library -- test and tuning knobs, none part of the drop-in surface -- as Markdown table rows
 * "| `NAME` | default | kind | what it does |" (csrc/yttm_config.h holds the one table; INTEGRATION.md prints it).  The hooks are read when a
 * trainer context or an encoder is created, never per round or per launch.  (No reference counterpart.) */
const char *yttm_config_table(void);

/* multi-GPU: attach a communicator (yttm_comm* from include/yttm_mi355x.h, passed as void*) before the stages run;
 * the context then holds ITS shard and the pair table holds GLOBAL counts */
int yttm_gpu_ctx_set_comm(yttm_ctx *ctx, void *comm);

/* corpus bytes: copy from host, or adopt a buffer already resident in HBM (16-byte aligned device pointer) */
int yttm_gpu_upload_corpus(yttm_ctx *ctx, const uint8_t *utf8, uint64_t n);
int yttm_gpu_attach_corpus(yttm_ctx *ctx, const void *device_ptr, uint64_t n);

/* K1 -- compute_char_count (bpe.cpp:839-857): histogram of valid non-space code points (*n_inout: capacity in,
 * count out; unsorted) and the number of decode steps (valid + invalid + space chars). */
int yttm_gpu_char_hist(yttm_ctx *ctx, uint32_t *cps, uint64_t *cnts, uint32_t *n_inout, uint64_t *n_codepoints);

/* K2 -- remove_rare_chars + compute_word_count + the layout half of build_linked_list (bpe.cpp:357-418, :436-451):
 * chars listed in cp[] map to compact ids id[]; every other non-space char is deleted; words = [space_id, ids...],
 * deduplicated exactly, stored as token tiles in HBM.  n_ids_cap = upper bound of token ids (vocab_size). */
int yttm_gpu_build_word_table(yttm_ctx *ctx, const uint32_t *cp, const uint32_t *id, uint32_t n_alpha, uint32_t space_id,
                              uint32_t n_ids_cap, uint64_t *n_unique, uint64_t *n_tokens);
/* test helper: current (compacted) word table; tok capacity = n_tokens, off = n_unique+1, cnt = n_unique */
int yttm_gpu_download_word_table(yttm_ctx *ctx, uint32_t *tok, uint64_t *off, uint32_t *cnt, uint64_t *n_tokens_now);

/* K3 -- pair2cnt of build_linked_list summed over shards (bpe.cpp:461-475, :1076-1088): weighted bigram histogram
 * into the HBM pair table (includes the cross-rank exchange on a multi-GPU context). */
int yttm_gpu_pair_count(yttm_ctx *ctx, uint64_t *n_pairs);
/* all pairs with count > 0 (unsorted); *n_inout: capacity in, count out */
int yttm_gpu_download_pairs(yttm_ctx *ctx, uint64_t *pairs /* x<<32|y */, uint64_t *counts, uint64_t *n_inout);
/* debug: the pair index of word mode as the rounds read it.  Key i is pairs[i] (unsorted), its postings -- class-A word rows, in no order,
 * duplicates allowed -- are post[run_lo[i] .. run_hi[i]).  *n_keys_inout, *n_post_inout: capacities in, counts out (also when the call fails
 * for lack of room, so that it can be repeated); both 0: no valid index.  Between rounds only, and like yttm_gpu_download_pairs it fails
 * while the scan of a yttm_gpu_merge_apply_scan is pending. */
int yttm_gpu_download_index(yttm_ctx *ctx, uint64_t *pairs, uint64_t *run_lo, uint64_t *run_hi, uint64_t *n_keys_inout, uint32_t *post,
                            uint64_t *n_post_inout);

/* K4 -- worker_doing_merge (bpe.cpp:491-812) for a batch of k mutually non-intersecting rules xyz[3k]
 * (rule_intersection, bpe.cpp:145-147; at most one x==y rule, last): applies them to every word and updates the
 * pair table exactly. */
int yttm_gpu_merge_apply(yttm_ctx *ctx, const uint32_t *xyz, uint32_t k);
/* The same round the way the trainer's merge loop runs it (host_trainer.cpp): rule_counts[k] are the pairs' exact global counts (what the
 * candidate filter returned for them), and the threshold of the candidate scan that will follow rides along -- next_want != 0: that scan
 * may raise the threshold to keep about so many candidates.  When the round's last launch can carry the scan (single GPU: hot and top
 * list active, no class-C tiles) the following yttm_gpu_candidates(next_tau_cnt, next_tau_mx) takes its answer from the mailbox instead
 * of scanning.
 * ORDER: the whole-table read-back of yttm_gpu_download_pairs lies over that mailbox, and until the scan's answer has been read the
 * host does not know whether the scan zeroed the batch's pairs (a scan that found its list overflowed did not).  So after this call
 * the next call that looks at the pair table must be yttm_gpu_candidates; yttm_gpu_download_pairs and yttm_gpu_pair_query in between
 * fail (they do not wait, and they do not disturb the pending scan).  yttm_gpu_download_word_table may come at any time. */
int yttm_gpu_merge_apply_scan(yttm_ctx *ctx, const uint32_t *xyz, uint32_t k, const uint64_t *rule_counts, uint64_t next_tau_cnt,
                              uint32_t next_tau_mx, uint32_t next_want);
/* Which paths the context's merge rounds and candidate scans took so far -- the counters of the training report, in this order:
 * [0] merge_rounds, [1] word_rounds, [2] word_all_rounds, [3] word_fused_rounds, [4] index_builds, [5] classb_word_rounds,
 * [6] fused_rounds, [7] fused_overflows, [8] hot_rebuilds, [9] top_refills, [10] word_switch_round, [11] exchange_retries (multi-GPU: rounds
 * whose exchange was repeated with wider blocks), [12] k3_radix (1: K3 counted class A by radix partition), [13] index_radix_builds (of
 * index_builds: filled by radix partition of the postings).  The first min(n, 14) go to out. */
#define YTTM_ROUND_STATS 14
int yttm_gpu_round_stats(yttm_ctx *ctx, uint64_t *out, uint32_t n);
/* Measurement mode of K4 (bench.py's untimed pass behind roofline.algorithmic_bytes_8d): on != 0 makes the following
 * yttm_gpu_merge_apply calls also count the WORDS that hold a merge site and their tokens (W_touched, T_touched).
 * out (optional) receives the totals so far: [0] merge sites, [1] tiles with a site, [2] their tokens, [3] words with a site,
 * [4] their tokens, [5] rounds. */
int yttm_gpu_k4_measure(yttm_ctx *ctx, int on, uint64_t out[6]);
/* check_cnt (bpe.cpp:1099-1108): exact global count of given pairs */
int yttm_gpu_pair_query(yttm_ctx *ctx, const uint64_t *pairs, uint32_t n, uint64_t *counts);
/* candidate filter feeding the host's ordered pick (PriorityQueue, bpe.cpp:271-314): pairs with count > tau_cnt, or
 * count == tau_cnt and max(x,y) <= tau_mx.  *n_inout: capacity in, number found out (may exceed capacity). */
int yttm_gpu_candidates(yttm_ctx *ctx, uint64_t tau_cnt, uint32_t tau_mx, uint64_t *pairs, uint64_t *counts, uint32_t *n_inout);

#ifdef __cplusplus
}
#endif
#endif
