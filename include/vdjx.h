/*
 * include/vdjx.h -- C ABI of libvdjx.so, the MI355X (gfx950) implementation of V'DJer's hot path.
 *
 * The reference (mozack/vdjer) has no plugin/FFI layer: it is one C++ program whose hot path is a
 * set of internal call sites.  Each entry point below replaces one of those call
 * sites; the "replaces:" lines cite the reference interface under /root/reference/src/main/c
 * (A2 = assembler2_vdj.c).  INTEGRATION.md shows the binding a maintainer adds on the reference side.
 *
 * Conventions: plain C types only; every call returns 0 on success or a negative VDJX_E* code with a
 * message available from vdjx_last_error(); nothing ever calls exit().  One host thread drives one
 * context; calls are synchronous (internally they run on the context's HIP stream).  Host pointers
 * unless a parameter is named d_* (device pointer, same device as the context).
 */
#ifndef VDJX_H
#define VDJX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VDJX_OK 0
#define VDJX_EINVAL (-1)   /* bad argument */
#define VDJX_EHIP (-2)     /* HIP runtime error */
#define VDJX_ELIMIT (-3)   /* input exceeds a documented limit: rl <= 160, k <= 50; 2^32 records in all (2^30 with reads of more than 64 bases); per GPU
                            * 2^29 records (2^27 with reads of more than 64 bases), 2^26 surviving k-mers, 2^26 - 1 distinct read sequences in the read index */
#define VDJX_ESTATE (-4)   /* call order violated (e.g. scorer used before its index was loaded) */

#define VDJX_MAX_READ_LEN 160   /* the reference takes up to 255 (bam_read.c:208 `char seq[256]`); reads of up to 64 bases run on the short-read kernels */
#define VDJX_SHORT_READ_LEN 64
#define VDJX_MAX_KMER 50    /* A2:70 MAX_KMER_LEN */

typedef struct vdjx_ctx vdjx_ctx;
typedef struct vdjx_pool vdjx_pool;
typedef struct vdjx_graph vdjx_graph;

const char* vdjx_last_error(void);
const char* vdjx_version(void);

/* One context per GPU (one process per GPU in multi-GPU runs). */
int vdjx_init(int device, vdjx_ctx** out);
void vdjx_shutdown(vdjx_ctx* ctx);
/* blocks until all work queued on the context's stream is done */
int vdjx_sync(vdjx_ctx* ctx);
/* gives the workspaces' device memory back (they hold the PEAK of the calls so far: tens of GB after a k-mer build of 10 M pairs) and with
 * them the scorers' grow-only result buffers (pair lists of the last window batch, mapped pairs and SAM records of the last contigs); the
 * next call maps again what it needs.  For a process that builds once and then serves scorer calls (a rank of `vdjer --gpus N`).  Not
 * between the two calls of a two-call protocol (vdjx_map_emit count / write, vdjx_window_pairs / _fetch), not during a sharded build. */
int vdjx_trim(vdjx_ctx* ctx);
/* drops the context's read index and frees its arrays (kept from build to build otherwise); the scorers need a new index afterwards */
int vdjx_read_index_drop(vdjx_ctx* ctx);
/* `bytes` bytes from one device buffer to another (synchronous): for drivers that move library-owned device results (vdjx_sam_blocks)
 * into exchange buffers of their own */
int vdjx_device_copy(vdjx_ctx* ctx, void* d_dst, const void* d_src, size_t bytes);

/* ---- a-0: read pool -------------------------------------------------------------------------
 * replaces: the two NUL-terminated ASCII pools handed to assemble() (A2:1350-1358, 1545-1554),
 * produced by add_to_buffer (bam_read.c:206-244): records of 2*rl+1 bytes, '0' + rl bases + rl
 * Phred+33 characters, primary pool scanned before secondary (A2:1388-1390).
 * Packs the pool on the device (2-bit bases A0 T1 C2 G3 as seq_to_kmer.c:6-29, N mask, Phred<20
 * mask, quality bytes).  Bases other than ACGT are treated as 'N'.  The caller keeps the ASCII. */
int vdjx_pool_load(vdjx_ctx* ctx, const uint8_t* primary, size_t n_primary,
                   const uint8_t* secondary, size_t n_secondary, int rl, vdjx_pool** out);
/* The same pools given as the reads only, n records of 2*rl+1 bytes as add_to_buffer writes the FIRST of each read's two
 * records (bam_read.c:219-230); the reverse-complement record it writes next (bam_read.c:231-243: complemented bases in reverse
 * order, reversed qualities) is derived on the device: record 2i is read i, record 2i+1 its reverse complement, half the bytes
 * cross PCIe.  The resulting pool is identical to vdjx_pool_load's on the full buffers. */
int vdjx_pool_load_forward(vdjx_ctx* ctx, const uint8_t* primary_reads, size_t n_primary_reads,
                           const uint8_t* secondary_reads, size_t n_secondary_reads, int rl, vdjx_pool** out);
/* vdjx_pool_load_forward without waiting: upload and packing run on the context's copy stream beside whatever the main stream is
 * computing on another pool (page-locked buffers, vdjx_host_alloc, make the upload a DMA); the pool may be used after vdjx_pool_wait,
 * which also reports a malformed pool. */
int vdjx_pool_load_forward_begin(vdjx_ctx* ctx, const uint8_t* primary_reads, size_t n_primary_reads,
                                 const uint8_t* secondary_reads, size_t n_secondary_reads, int rl, vdjx_pool** out);
int vdjx_pool_wait(vdjx_pool* pool);
/* The reads in a PACKED host format, for callers that can produce it (an extraction that converts BAM's 4-bit bases itself): per read
 * vdjx_packed_read_bytes(rl) bytes -- ceil(rl/4) bytes of 2-bit bases (A0 T1 C2 G3 as seq_to_kmer.c:6-29, the first base in the top two
 * bits of byte 0, code 0 for a base that is not ACGT), then rl quality bytes (Phred+33, bit 7 set where the base is not ACGT), zero
 * padding to a multiple of 16: 64 bytes for a 50 bp read where add_to_buffer's record (bam_read.c:219-230) has 101 -- 128 bytes per
 * pair over PCIe instead of 202.  Reads of up to 64 bases.  Otherwise exactly vdjx_pool_load_forward[_begin]: record 2i is read i,
 * record 2i+1 its reverse complement with reversed qualities.  vdjx_pack_reads converts n ASCII records on the host (plain C). */
size_t vdjx_packed_read_bytes(int rl);
int vdjx_pack_reads(const uint8_t* ascii_reads, size_t n, int rl, uint8_t* out_packed);
int vdjx_pool_load_packed(vdjx_ctx* ctx, const uint8_t* primary_reads, size_t n_primary_reads,
                          const uint8_t* secondary_reads, size_t n_secondary_reads, int rl, vdjx_pool** out);
int vdjx_pool_load_packed_begin(vdjx_ctx* ctx, const uint8_t* primary_reads, size_t n_primary_reads,
                                const uint8_t* secondary_reads, size_t n_secondary_reads, int rl, vdjx_pool** out);
/* same, ASCII pools already resident in device memory (16-byte aligned).  The two buffers must stay valid and unchanged until
 * vdjx_pool_free: bases and masks are packed, but the quality characters are NOT copied -- the few k-mers whose quality sums
 * matter (count below 1 + ceil(mq/20), A2:454-465) read them from the records where they lie (a third of the packing's bytes). */
int vdjx_pool_load_device(vdjx_ctx* ctx, const uint8_t* d_primary, size_t n_primary,
                          const uint8_t* d_secondary, size_t n_secondary, int rl, vdjx_pool** out);
size_t vdjx_pool_records(const vdjx_pool* pool);
void vdjx_pool_free(vdjx_pool* pool);

/* ---- a-6: V/J anchor sets ---------------------------------------------------------------------
 * replaces: vjf_init -> load_kmers (vj_filter.c:56-68, 311-340): the codes whose distance column
 * passed --am.  Kept as two 2^32-bit bitmaps in HBM; code 0 is never a member (vj_filter.c:317-318). */
int vdjx_anchor_sets_load(vdjx_ctx* ctx, const uint32_t* v_codes, size_t nv, const uint32_t* j_codes, size_t nj);
/* replaces: seq_to_int + matches_vmer/matches_jmer over every offset of a contig
 * (vj_filter.c:221-238): out_v/out_j[i] for i in [0, len-16) */
int vdjx_anchor_probe(vdjx_ctx* ctx, const char* contig, int len, uint8_t* out_v, uint8_t* out_j);

/* ---- a-1, a-2, a-3: k-mer table, prune, graph build --------------------------------------------
 * replaces: build_pre_graph x2 + prune_pre_graph + build_graph2 x2 (A2:1388-1408; bodies
 * A2:240-259, 322-367, 454-484, 267-320, 190-237).  The result is everything the host-side
 * traversal needs without re-scanning the pool: nodes in creation order with their ordered edge
 * lists. */
int vdjx_kmer_build(vdjx_ctx* ctx, const vdjx_pool* pool, int k, int mf, int mq, vdjx_graph** out);
size_t vdjx_graph_nodes(const vdjx_graph* g);
/* distinct gated k-mers before the prune ("Pre Num nodes", A2:407) */
size_t vdjx_graph_pre_nodes(const vdjx_graph* g);
/* Node i (0-based; reference node id = i+1, A2:188,200), in creation order:
 *   first_inst  record << 6 | offset of the first (ungated) occurrence, records counted over primary then secondary
 *               (pools of reads longer than 64 bases: record << 8 | offset)
 *   gated_count frequency of the pre_node (A2:130,345-347), saturated at 32765
 *   freq        node frequency (A2:119,261-265), saturated at 32765
 *   has_v/has_j A2:288-303
 *   to_deg/from_deg <= 4; to_ids/from_ids [n][4] 1-based node ids in list order (head of the
 *   reference's prepend list first, A2:223-237)
 *   kmers       n*k ASCII characters (may be NULL)                                              */
int vdjx_graph_export(const vdjx_graph* g, uint64_t* first_inst, uint32_t* gated_count, uint32_t* freq,
                      uint8_t* has_v, uint8_t* has_j, uint8_t* to_deg, uint32_t* to_ids,
                      uint8_t* from_deg, uint32_t* from_ids, char* kmers);
/* the same copies started on a second stream: they run beside whatever is done next with the context (e.g. vdjx_root_score_graph
 * on the device-resident graph); the arrays are valid after vdjx_graph_export_end.  Pinned arrays (vdjx_host_alloc) make it a DMA. */
int vdjx_graph_export_begin(const vdjx_graph* g, uint64_t* first_inst, uint32_t* gated_count, uint32_t* freq,
                            uint8_t* has_v, uint8_t* has_j, uint8_t* to_deg, uint32_t* to_ids,
                            uint8_t* from_deg, uint32_t* from_ids, char* kmers);
/* The ten arrays lie in one block on the device.  offsets[10]: where each starts in it, in the order of vdjx_graph_export's arguments
 * (every array holds vdjx_graph_nodes entries; ids in rows of 4, k-mers in rows of k); *bytes: the bytes that hold them all.
 * vdjx_graph_export_block copies those bytes into host_block (same layout) in ONE transfer; _begin does it on the second stream
 * (vdjx_graph_export_end waits).  For callers that export small graphs often: ten transfers cost more in calls than in bytes. */
int vdjx_graph_block_layout(const vdjx_graph* g, uint64_t* offsets, uint64_t* bytes);
int vdjx_graph_export_block(const vdjx_graph* g, void* host_block);
int vdjx_graph_export_block_begin(const vdjx_graph* g, void* host_block);
int vdjx_graph_export_end(const vdjx_graph* g);
void vdjx_graph_free(vdjx_graph* g);

/* ---- f-3: the v_index / j_index generator -------------------------------------------------------
 * replaces: process_kmers(anchors file, start, end) (seq_dist.c:49-71; its main() is commented out, :73-98) which
 * printed "<code>\t<min base distance to any anchor>" for every 16-base code of [start, end] (inclusive) whose
 * distance is <= MAX_DIST 5: the rows of <ref-dir>/v_index and j_index (load_kmers, vj_filter.c:56-68).
 * anchors: seq_to_int codes of the anchor 16-mers.  Rows come in ascending code order; *n_rows = how many
 * exist, the first min(cap, *n_rows) are written (call with cap 0 to count).                           */
int vdjx_index_generate(vdjx_ctx* ctx, const uint32_t* anchors, size_t n_anchors, uint64_t start, uint64_t end, int max_dist,
                        uint64_t cap, uint64_t* n_rows, uint32_t* codes, uint8_t* dists);
/* The two membership sets of a-6 straight from the anchors, without 10^7..10^8-row files in between: exactly the sets
 * vdjx_anchor_sets_load would hold after load_kmers(v_index, am) / load_kmers(j_index, am) on generated files
 * (distance <= min(am, 5); code 0 never a member).                                                   */
int vdjx_anchor_sets_from_anchors(vdjx_ctx* ctx, const uint32_t* v_anchors, size_t nv, const uint32_t* j_anchors, size_t nj, int am);

/* ---- result buffers ------------------------------------------------------------------------------
 * Every result pointer of this interface may be ordinary host memory.  Memory from vdjx_host_alloc is
 * page-locked: copies into it run at DMA speed (the graph of 1 M pairs is ~11 MB, the mapped pairs ~11 MB).
 * Windows / contigs handed to the scorers in such memory are not copied at all: the classifying kernel reads them where they lie
 * (each character once, over PCIe), and they must stay unchanged until the call returns -- as for any argument.
 * No counterpart in the reference (its tables are host memory throughout).                          */
int vdjx_host_alloc(vdjx_ctx* ctx, size_t bytes, void** out);
void vdjx_host_free(vdjx_ctx* ctx, void* p);
/* dst row i = bytes [first, first + len) of src row idx[i] (rows `stride` bytes apart): the contigs of the accepted windows, laid
 * end to end for vdjx_map_emit (output_windows hands the [51,411) slice of a window that passed coverage on, A2:841-847,872-914). */
int vdjx_host_take_rows(void* dst, const void* src, size_t stride, size_t first, size_t len, const uint32_t* idx, size_t n);

/* ---- a-7: root (V-region homology) scorer ------------------------------------------------------
 * replaces: score_seq_init(k, 1000, v_region.fa) (seq_score.c:50-70) and score_seq(kmer, thr)
 * (seq_score.c:118-158) as called per root by worker_thread (A2:1103).
 * lines: the non-header lines of v_region.fa, newline stripped; each must be longer than 2k.     */
int vdjx_vregion_load(vdjx_ctx* ctx, const char* const* lines, size_t n_lines, int vk);
/* kmers: n*k ASCII; out[i] = 0|1 */
int vdjx_root_score(vdjx_ctx* ctx, const char* kmers, size_t n, int k, int threshold, uint8_t* out);
/* The same scorer over the roots of a graph that is still on the device (identify_root_nodes, A2:653-676: the nodes
 * without predecessor), so that root k-mers never travel to the host and back.  vdjx_graph_roots = their number;
 * roots are taken in ascending node id, this call handles the ones at positions first, first+stride, ...
 * (vdjx_root_part of them: one call with (0,1) on one GPU, (rank,nranks) when sharded).
 * root_ids[i] = 1-based node id, out[i] = 0|1.                                                    */
size_t vdjx_graph_roots(const vdjx_graph* g);
size_t vdjx_root_part(const vdjx_graph* g, uint32_t first, uint32_t stride);
int vdjx_root_score_graph(vdjx_ctx* ctx, const vdjx_graph* g, int threshold, uint32_t first, uint32_t stride,
                          uint32_t* root_ids, uint8_t* out);
/* The same without waiting: everything is queued on the context's stream and the call returns; the two arrays (page-locked memory,
 * vdjx_host_alloc) are valid after vdjx_root_score_graph_end.  Calls made in between run behind it on the device, so a caller with
 * other work that does not need the verdicts (scoring windows it already has) keeps the device busy instead of waiting for a few
 * kilobytes.  The graph stays alive until _end; one call in flight per context. */
int vdjx_root_score_graph_begin(vdjx_ctx* ctx, const vdjx_graph* g, int threshold, uint32_t first, uint32_t stride,
                                uint32_t* root_ids, uint8_t* out);
int vdjx_root_score_graph_end(vdjx_ctx* ctx);

/* ---- a-8, a-9, a-10: read->contig mapper, coverage validator, SAM placements --------------------
 * replaces: add_read_info (quick_map3.c:126-149) for the index; quick_map_process_contig +
 * coverage_is_valid as called per candidate window by output_contig (A2:841-847; quick_map3.c:188-266,
 * coverage.c:10-130); quick_map_process_contig_file -> output_mapping for the final contigs
 * (quick_map3.c:152-181, 311-340).
 * Per pool record (scan order): pair id (identity of the read name), read_num 1|2, is_rc, and the
 * registration rank (order of the add_read_info calls).                                           */
int vdjx_read_index_build(vdjx_ctx* ctx, const vdjx_pool* pool, const uint32_t* pair_id,
                          const uint8_t* read_num, const uint8_t* is_rc, const uint32_t* reg_rank, uint32_t n_pairs);
/* the same with the four per-record arrays already in device memory (e.g. written there by the extraction side) */
int vdjx_read_index_build_device(vdjx_ctx* ctx, const vdjx_pool* pool, const uint32_t* d_pair_id,
                                 const uint8_t* d_read_num, const uint8_t* d_is_rc, const uint32_t* d_reg_rank, uint32_t n_pairs);

/* The same two calls begun and ended: the index is built on a stream and out of a workspace of its own, by a thread of the library,
 * BESIDE whatever the caller does next with the context -- the k-mer build of the same pool above all: both only read the packed
 * records, and the reference orders them only by accident of its call sequence (add_read_info runs inside extract, bam_read.c:228,243,
 * before A2:1388; nothing reads the index before the first quick_map_process_contig, A2:841).  Everything queued on the context
 * before _begin comes first (the packing of `pool`; scorer calls that still read the index being replaced).  _end returns the
 * build's status; the first call that needs the index (vdjx_window_score, vdjx_window_pairs, vdjx_map_emit, vdjx_sam_text ...) ends a
 * build that was not.  _begin (host arrays): the four arrays must stay valid until _end.  One build in flight per context; `pool`
 * may not be freed before _end (vdjx_pool_free waits for it). */
int vdjx_read_index_build_begin(vdjx_ctx* ctx, const vdjx_pool* pool, const uint32_t* pair_id,
                                const uint8_t* read_num, const uint8_t* is_rc, const uint32_t* reg_rank, uint32_t n_pairs);
int vdjx_read_index_build_device_begin(vdjx_ctx* ctx, const vdjx_pool* pool, const uint32_t* d_pair_id,
                                       const uint8_t* d_read_num, const uint8_t* d_is_rc, const uint32_t* d_reg_rank, uint32_t n_pairs);
int vdjx_read_index_build_end(vdjx_ctx* ctx);

typedef struct {
	int eval_start;    /* --e0 */
	int eval_stop;     /* --e1 */
	int read_span;     /* --rs */
	int mate_span;     /* --ms */
	int insert_low;    /* --ins */
	int insert_high;   /* --ins */
	int floor;         /* --rf; 0 disables the coverage check (A2:846) */
} vdjx_cov_params;

/* windows: n strings of `len` chars, stride `len`.  out_valid[i] = coverage_is_valid(...),
 * out_npairs[i] = mapped pairs.  Any n: the windows' pair lists (8 bytes per distinct hit) are built in device memory, and a call
 * whose lists would not fit takes its windows in slices (vdjx_stat "window_slices"); one window's lists have to fit. */
int vdjx_window_score(vdjx_ctx* ctx, const char* windows, size_t n, int len, const vdjx_cov_params* p,
                      uint8_t* out_valid, uint32_t* out_npairs);

/* The two halves of vdjx_window_score, for a read index that holds only this rank's share of the pairs (multi-GPU: the pool is
 * split BY PAIR, both mates of a pair on one rank).  Every rank maps every window against its own reads:
 *   vdjx_window_pairs        out_entries[i] = entries of window i's pair list (identical read pairs are one entry with a
 *                            multiplicity), out_npairs[i] = mapped pairs (quick_map3.c:223-245); the lists stay on the device
 *   vdjx_window_pairs_fetch  the lists of the m named windows laid end to end (8 bytes per entry) into d_out: what travels
 *                            to the ranks that own those windows
 * and the owner of a window tests the union of what all ranks found (coverage_is_valid only counts entries, coverage.c:64-130):
 *   vdjx_window_cover        d_lists = the lists as received: source after source, inside a source window after window;
 *                            counts[s*n + w] = entries of window w from source s; an entry is
 *                            multiplicity << 32 | pos1 << 16 | pos2, positions in 1 .. len - rl.  Refused ("bad geometry") unless
 *                            1 <= rl <= VDJX_MAX_READ_LEN, rl < len <= 1024 + rl and nsrc >= 1                          */
int vdjx_window_pairs(vdjx_ctx* ctx, const char* windows, size_t n, int len, uint32_t* out_entries, uint32_t* out_npairs);
int vdjx_window_pairs_fetch(vdjx_ctx* ctx, const uint32_t* window_ids, size_t m, void* d_out);
int vdjx_window_cover(vdjx_ctx* ctx, size_t n, int len, int rl, const vdjx_cov_params* p, const void* d_lists, size_t nsrc,
                      const uint32_t* counts, uint8_t* out_valid);

typedef struct {
	uint32_t pair_id;
	uint32_t rec1, rec2;       /* pool record (scan order) that matched for read 1 / read 2 */
	int16_t pos1, pos2, insert;
	uint8_t rc1, rc2;
} vdjx_pair;

/* Mapped pairs of each contig in the reference's output order.  Two-call protocol: first call with
 * pairs == NULL fills offsets[n+1]; second call with pairs sized offsets[n]. */
int vdjx_map_emit(vdjx_ctx* ctx, const char* contigs, size_t n, int len, uint64_t* offsets, vdjx_pair* pairs);
/* The writing call with the transfer to the host left running on the context's copy stream (page-locked `pairs`, vdjx_host_alloc,
 * make it a DMA beside the next kernels); the array is valid after vdjx_map_emit_end. */
int vdjx_map_emit_begin(vdjx_ctx* ctx, const char* contigs, size_t n, int len, uint64_t* offsets, vdjx_pair* pairs);
int vdjx_map_emit_end(vdjx_ctx* ctx);

/* The SAM records themselves, formatted on the device.
 * replaces: output_mapping (quick_map3.c:152-181) as called through quick_map_process_contig_file (:311-340): per mapped pair the two
 * lines "%s\t%d\t%s\t%d\t255\t%dM\t=\t%d\t%d\t%s\t%s\n" (:168) -- read name without its leading '@', flag, contig id, position, read
 * length, mate position, insert, then the stored sequence and qualities of the record that matched -- contig after contig, in the order
 * of vdjx_map_emit.  (The header lines, output_header :274-309, are the caller's: they need only the contig ids.)
 *   vdjx_sam_names_load  the read names by pair id (the pair_id of vdjx_read_index_build): names[name_off[p] .. name_off[p+1])
 *   vdjx_sam_text        contig ids likewise (ids[id_off[c] .. id_off[c+1])); *out_text points at *out_bytes bytes (NUL after them) in a
 *                        page-locked buffer owned by the context, valid until the next vdjx_sam_text call
 * Bases that are not ACGT come out as N (they are stored as N: see vdjx_pool_load).                                                   */
int vdjx_sam_names_load(vdjx_ctx* ctx, const char* names, const uint64_t* name_off, uint32_t n_pairs);
int vdjx_sam_text(vdjx_ctx* ctx, const char* contigs, size_t n, int len, const char* ids, const uint32_t* id_off,
                  const char** out_text, uint64_t* out_bytes);

/* ---- the same records for a pool that is sharded BY PAIR over several GPUs (row e; no counterpart in the reference) -----------------
 * Every rank formats the records of ITS pairs and leaves them on its device; the caller brings the ranks' results to one rank, which
 * lays them out in the order output_mapping would have written them (quick_map3.c:152-181 called per contig from :311-340; inside a
 * contig the order of quick_map_process_contig's lists, :199-245: offsets ascending, the instances of a read in registration order).
 *   vdjx_sam_blocks   maps `contigs` against this context's read index; per mapped pair ("block") the two SAM lines, their byte
 *                     count (u32) and a 64-bit key (contig << 44 | read-1 position << 32 | registration rank of the read-1 record;
 *                     d_reg_rank: the rank of every record of the index's pool, GLOBAL over all shards).  The three arrays stay on the
 *                     device, owned by the context, valid until the next vdjx_sam_blocks / vdjx_sam_text call.  Fewer than 2^20 contigs
 *                     of fewer than 4096 bases per call.
 *   vdjx_sam_merge    d_keys / d_lens / d_text = the blocks of all sources, source after source (every source's text the concatenation of
 *                     its blocks in its own order); *out_text = the n_bytes of text in ascending key order, in a page-locked buffer owned
 *                     by the context, valid until the next vdjx_sam_merge call.                                                   */
int vdjx_sam_blocks(vdjx_ctx* ctx, const char* contigs, size_t n, int len, const char* ids, const uint32_t* id_off, const uint32_t* d_reg_rank,
                    uint64_t* n_blocks, uint64_t* n_bytes, const void** d_keys, const void** d_lens, const void** d_text);
int vdjx_sam_merge(vdjx_ctx* ctx, uint64_t n_blocks, uint64_t n_bytes, const void* d_keys, const void* d_lens, const void* d_text,
                   const char** out_text, uint64_t* out_bytes);
/* ---- contig abundances: the step the reference's workflow runs after every vdjer run ---------------------------------------------
 * replaces: `samtools view -bS vdjer.sam`, a name sort, `rsem-prepare-reference vdj_contigs.fa` and `rsem-calculate-expression
 * --paired-end` (demo/quant_demo.bash; post_process/post_processing.readme.txt), of whose output post_process/collect_vdjer_stats.py
 * reads only expected_count.  The placements are vdjx_map_emit's pairs for `contigs` (the SAM records of vdjx_sam_text), kept on the
 * device; every placement of a pair is one alignment.  RSEM's core paired-end model in float64:
 *   fragment lengths  P(f) = (h(f) + 1) / sum(h + 1) over f in [50, 400] (MIN_INSERT / MAX_INSERT, quick_map3.c:23-24), h = inserts of
 *                     the pairs placed exactly once; an alignment of insert f weighs g(f) = P(f) / (len - f + 1)
 *   start             N_c = placed pairs / contigs with a placement (0 for the others, for good)
 *   iteration         E: r_a = N_c(a) g(f_a) / sum over the pair's alignments;  M: N_c = sum of r_a over the alignments on c
 *   stop              after iteration t when max_c |N_c(t) - N_c(t-1)| / max(N_c(t), 1) < tol, or at t = max_iter (tol 0: max_iter)
 * out_counts[n] = N (RSEM's expected_count; TPM, FPKM and IsoPct follow from it and info->eff_len = sum_{f <= len} P(f) (len - f + 1)).
 * NOT modelled: RSEM's noise transcript, read qualities and mismatches (a placement here is exact), fragment-length tails outside
 * [50, 400], Gibbs sampling and credibility intervals (vdjx_quant_boot below bootstraps the counts instead), gene-level grouping (every
 * contig is its own gene).  Bitwise reproducible
 * (no floating-point atomics).  n = 0 and pools that place no pair give zeros.  Contigs of unequal length (a NUL inside the n*len
 * characters), max_iter < 1 and tol < 0 are VDJX_EINVAL; fewer than 2^20 contigs of fewer than 4096 bases per call (vdjx_sam_blocks'
 * limit).  Scratch comes from the context's workspace; the text of an earlier vdjx_sam_text stays valid.  One GPU only (a pool sharded
 * by pair would need a per-iteration all-reduce of N). */
typedef struct { int max_iter; double tol; } vdjx_quant_params;
typedef struct { uint64_t pairs, alignments, unique_pairs; uint32_t iterations, converged; double eff_len; } vdjx_quant_info;
int vdjx_quant(vdjx_ctx* ctx, const char* contigs, size_t n, int len, const vdjx_quant_params* params, double* out_counts, vdjx_quant_info* info);
/* The same model over placements the caller brings, in the shape vdjx_map_emit returns them: contig-major, offsets[n + 1] with
 * offsets[0] = 0 and no decrease, pairs[offsets[n]]; contig c holds pairs[offsets[c] .. offsets[c + 1]).  Of a vdjx_pair only pair_id and
 * insert are read.  Every pair_id < n_pairs (ids without a placement are skipped); an insert may be any int16, and those outside
 * [50, min(400, len)] weigh 0 (a pair all of whose alignments weigh 0 adds nothing to any contig).  No pool and no read index are needed;
 * the placements are copied into the context's workspace and nothing is kept.  Output, info and bits are vdjx_quant's for the same
 * placements; the stat "quant_map_us" is 0.  VDJX_EINVAL: a NULL argument, offsets[0] != 0, offsets that decrease, a pair_id >= n_pairs,
 * max_iter < 1, tol negative or NaN, len < 1.  VDJX_ELIMIT: n >= 2^20, len >= 4096, offsets[n] >= 2^32.  n = 0 and offsets[n] = 0 give
 * zeros, converged = 1 and the eff_len of a histogram without counts. */
int vdjx_quant_pairs(vdjx_ctx* ctx, const uint64_t* offsets, const vdjx_pair* pairs, size_t n, int len, uint32_t n_pairs,
                     const vdjx_quant_params* params, double* out_counts, vdjx_quant_info* info);
/* ---- the bootstrap of the abundances: what `rsem-calculate-expression --calc-ci` (kallisto's and salmon's bootstrap) adds to the table
 * The bootstrap is over the placed pairs, everything else held fixed (kallisto's bootstrap):
 *   slots             the placed pairs in ascending pair id are the slots q = 0 .. Pp - 1 (vdjx_quant's pair-major order)
 *   multiplicities    replicate r (1 .. B) draws Pp times; draw i (0 .. Pp - 1) falls on slot hi64(mix64(mix64(seed) + (r << 32 | i)) * Pp),
 *                     vdjx_diversity's draw rule with W = Pp; m_r[q] = the draws on slot q, counted exactly in uint32 (integer atomics)
 *   fixed inputs      the point estimate's, from the original sample: P(f), g(f), eff_len and the start value N_c = Pp / contigs with
 *                     a placement
 *   iteration         E: r_a = N_c(a) g(f_a) / sum over the pair's alignments (unchanged);  M: N_c = sum over the alignments a on c of
 *                     m_r[pair(a)] * r_a
 *   stop              vdjx_quant's rule, per replicate, with an iteration count of its own (tol 0: max_iter iterations)
 * No floating-point atomics: a replicate's N is a fixed function of (placements, seed, r, max_iter, tol); its bits do not depend on the
 * batch it ran in, on how many replicates shared the batch, or on the call before.  out_counts and info are vdjx_quant's for the same
 * input, bit for bit; out_boot[B * n] is replicate-major (row r - 1 is replicate r), out_iters[B] the iterations of every replicate.
 * boot_info: converged = replicates whose last delta was below tol, batches, max_iterations = the most iterations of a replicate,
 * iterations = their sum.  The replicates run in batches of max(1, floor(VDJX_QBOOT_CELLS / (pairs + n))) whole replicates (a replicate
 * takes a cell per placed pair and per contig).  VDJX_EINVAL: replicates outside 1 .. 1024, and everything vdjx_quant refuses;
 * VDJX_ELIMIT: replicates * n >= 2^27, and vdjx_quant's limits.  n = 0 and pools that place no pair give zeros, iterations 0 and
 * converged = replicates.  Scratch comes from the context's workspace; nothing more is kept on the device.  Stats: "quant_boot_us",
 * "quant_boot_em_us" (host clock).  NOT modelled: a resampled fragment-length distribution (P(f) is the original sample's), Gibbs
 * sampling, intervals for TPM / FPKM.
 * vdjx_quant_pairs_boot: the same over the caller's placements (vdjx_quant_pairs' arguments and refusals).  mult (NULL, or B * n_pairs
 * by replicate and pair id): the draws are skipped and m_r[q] is read from the caller -- a weighted EM; entries of ids without a
 * placement are ignored, a replicate whose placed multiplicities sum to 2^32 or more is VDJX_EINVAL.  out_mult (NULL, or B * n_pairs):
 * the multiplicities used, 0 for ids without a placement.
 * vdjx_quant_boot_summary (plain C, no GPU): per contig of a B x n replicate-major matrix, mean = the replicates added in the order
 * r = 1 .. B over B; sd = sqrt(sum (x_r - mean)^2 / (B - 1)) in the same order, 0 at B = 1; with v the B values sorted ascending,
 * lower = v[floor(25 (B - 1) / 1000)] and upper = v[ceil(975 (B - 1) / 1000)] (integer arithmetic: the 2.5 % and 97.5 % order
 * statistics).  An output that is NULL is left out. */
typedef struct { int replicates; uint64_t seed; } vdjx_quant_boot_params;
typedef struct { uint32_t replicates, converged, batches, max_iterations; uint64_t iterations; } vdjx_quant_boot_info;
int vdjx_quant_boot(vdjx_ctx* ctx, const char* contigs, size_t n, int len, const vdjx_quant_params* params, const vdjx_quant_boot_params* boot_params,
                    double* out_counts, vdjx_quant_info* info, double* out_boot, uint32_t* out_iters, vdjx_quant_boot_info* boot_info);
int vdjx_quant_pairs_boot(vdjx_ctx* ctx, const uint64_t* offsets, const vdjx_pair* pairs, size_t n, int len, uint32_t n_pairs,
                          const vdjx_quant_params* params, const vdjx_quant_boot_params* boot_params, const uint32_t* mult, uint32_t* out_mult,
                          double* out_counts, vdjx_quant_info* info, double* out_boot, uint32_t* out_iters, vdjx_quant_boot_info* boot_info);
void vdjx_quant_boot_summary(const double* boot, uint32_t B, size_t n, double* mean, double* sd, double* lower, double* upper);

/* ---- contig annotation: V/J calls, identity and CIGARs against the germline segments (the ref-dir's ig_vdj.fa) -----------------------
 * replaces the IMGT HighV-QUEST round trip of the reference's post_process/ (collect_vdjer_stats.py reads the V gene, the J gene, the
 * V-region identity and the CDR3 from it).  All arithmetic is integer: the device's results are bitwise the model's.
 *   germlines   vdjx_germline_load: record r is seqs[off[r] .. off[r+1]) of class cls[r] ('V', 'J'; anything else is counted and
 *               skipped).  The caller parses the FASTA: the name is the header's first token, or its second '|' field when the token has
 *               one (IMGT/GENE-DB); the class is the name's 4th character for IG[HKL]* / TR[ABDG]* names, its 1st otherwise; sequences
 *               uppercased, '.' and whitespace dropped.  The set stays on the device until the next load or vdjx_shutdown.
 *   scoring     Smith-Waterman with affine gaps (Gotoh), contig row i in 1..m, germline column j in 1..g; a gap of k bases costs
 *               open + k ext; s(i,j) = +match when both bases are equal and in ACGT (upper case), -mismatch otherwise (N included):
 *                 E[i][j] = max(E[i][j-1] - ext, H[i][j-1] - open - ext)     (D: germline base j missing from the contig)
 *                 F[i][j] = max(F[i-1][j] - ext, H[i-1][j] - open - ext)     (I: contig base i not in the germline)
 *                 H[i][j] = max(0, H[i-1][j-1] + s(i,j), E[i][j], F[i][j]);  H = 0 on row 0 and column 0, E = F = -inf there
 *   score       S = max H; the end cell is the first cell in row-major order (smallest i, then smallest j) that holds S
 *   calls       per class: the primary hit is the germline of highest S, the lowest record index on a tie; n_tied counts the germlines at
 *               that S and tied[] lists the first 8 of them in index order (AIRR's comma-joined v_call).  No call (gene -1, n_tied 0)
 *               when S < min_v_score / min_j_score, or when the class has no record; score is S all the same.
 *   traceback   the primary hit only, from the end cell in state H:
 *                 H at (i,j): H == 0: stop (the alignment begins at (i+1, j+1)); H == H[i-1][j-1] + s: align, to H (i-1,j-1);
 *                             else H == E: to E at (i,j); else to F at (i,j)
 *                 E: emit D; E[i][j] == H[i][j-1] - open - ext (a gap open): to H (i,j-1), else to E (i,j-1)
 *                 F: emit I; F[i][j] == H[i-1][j] - open - ext (a gap open): to H (i-1,j), else to F (i-1,j)
 *               seq_/germ_start and _end are 1-based closed; matches + mismatches are the aligned pairs; ins / del the I / D bases; opens
 *               the gap opens the traceback took (so S = match*matches - mismatch*mismatches - open*opens - ext*(ins + del)).  runs[] are
 *               the M/I/D runs 5' to 3' as len << 4 | op (op 0 M, 1 I, 2 D: BAM's codes); n_runs counts them all, runs[] holds them only
 *               when n_runs <= 64 (otherwise zeros: the CIGAR is written empty, stat "annot_cigar_truncated").  S = 0: no traceback
 *               (coordinates and counts 0).  identity = matches / (matches + mismatches + ins + del).
 * NOT modelled: IMGT gaps and numbering (the ungapped sequence_alignment / germline_alignment rows are vdjx_mutations' below: `vdjer
 * --mutations` fills the two AIRR cells); reverse-complement contigs (a contig is always V to J);
 * IgBLAST's or V-QUEST's own identity definitions.  The isotype is a call of its own against a constant-region set (vdjx_isotype below),
 * the D gene a call of its own against the D records, between the V and the J hit (vdjx_dcall below).
 * VDJX_EINVAL: contigs of unequal length (a NUL inside the n*len characters), len >= 4096, a V/J germline of 0 or >= 2048 bases, 2^20
 * records or more, match outside 1..15 or mismatch / gap_open / gap_extend outside 0..31 (every H then fits int16); vdjx_annotate before
 * any vdjx_germline_load is VDJX_ESTATE.  n = 0 returns at once.  Scratch comes from the context's workspace; no floating-point atomics,
 * two runs are bitwise equal.  VDJX_ANNOT_PAIRS (environment, read once): (contig, germline) pairs per scoring launch. */
#define VDJX_ANNOT_TIED 8
#define VDJX_ANNOT_RUNS 64
typedef struct { int match, mismatch, gap_open, gap_extend, min_v_score, min_j_score; } vdjx_annot_params;
typedef struct {
	int32_t gene, score, n_tied, tied[VDJX_ANNOT_TIED];
	int32_t seq_start, seq_end, germ_start, germ_end;
	int32_t matches, mismatches, ins, del, opens, n_runs;
	uint32_t runs[VDJX_ANNOT_RUNS];
} vdjx_annot_hit;                                              /* 340 bytes */
int vdjx_germline_load(vdjx_ctx* ctx, const char* seqs, const uint64_t* off, const char* cls, size_t n);
int vdjx_annotate(vdjx_ctx* ctx, const char* contigs, size_t n, int len, const vdjx_annot_params* params, vdjx_annot_hit* out_v,
                  vdjx_annot_hit* out_j);

/* ---- isotype calls: the contigs' 3' ends against the constant regions ------------------------------------------------------------------
 * replaces the isotype step of the reference's post_process/ (call_isotypes.bash: get_cseq.py cuts the last 48 bases of every contig,
 * isotypes_star.bash maps them to the whole genome with STAR, call_isotypes.py looks the hit up in igh_constant_func.bed) by a local
 * alignment against the constant-region sequences themselves.  All arithmetic is integer: the device's results are bitwise the model's.
 *   constants   vdjx_constant_load: record r is seqs[off[r] .. off[r+1]), cleaned by the caller exactly as for vdjx_germline_load (upper
 *               case, '.' and whitespace dropped).  Every record is a constant record whatever its name.  0 .. 4096 records of 1 .. 2047
 *               bases.  The set lives in a device buffer of its own, independent of the germline set, until the next
 *               vdjx_constant_load or vdjx_shutdown.
 *   query       the tail of a contig: its last T = min(tail, len) bases, tail in 16 .. 64 (48: get_cseq.py).  (64: one wave holds one
 *               tail row per lane.)
 *   score       vdjx_annotate's recurrences and scoring rule, unchanged (Gotoh, integer, N never matches), tail row i in 1..T, record
 *               r's column j in 1..g_r: S(contig, r) = max H.  out_scores (may be NULL) receives every S, out_scores[contig * C + r]
 *               (a runner-up score is what tells IGHG1 from IGHG2).
 *   call        the primary hit is the record of highest S, the lowest index on a tie; n_tied counts the records at that S and tied[]
 *               lists the first 8 of them in index order.  No call (gene -1, n_tied 0, tied[] -1) when S < min_score or C = 0; score is
 *               S all the same (0 when C = 0).
 *   traceback   the primary hit only, by vdjx_annotate's rules and preference order (the end cell: the first in row-major order that
 *               holds S); every field of vdjx_annot_hit means what it means there.  seq_start / seq_end are in CONTIG coordinates (tail
 *               coordinate + len - T); S = 0: no traceback.
 * Defaults (what `vdjer --isotypes` uses): match 2, mismatch 3, gap_open 5, gap_extend 2, min_score 48, tail 48.  min_score 48 is half
 * the score of a perfect 48-base tail: 400 random 48-mers against 9 random records of 1,000 bases reach at most 29 (median 19), a true
 * tail with three substitutions scores 81.  It is a parameter of the model, not a tolerance.
 * VDJX_EINVAL: contigs of unequal length (a NUL inside the n*len characters), len >= 4096, n >= 2^20, tail outside 16 .. 64, match
 * outside 1..15 or mismatch / gap_open / gap_extend outside 0..31, min_score < 0; more than 4096 records or a record of 0 or >= 2048
 * bases (vdjx_constant_load).  vdjx_isotype before any vdjx_constant_load is VDJX_ESTATE.  n = 0 returns at once.  Scratch (the score
 * matrix included) comes from the context's workspace; no floating point, no atomics: two calls give the same bits. */
typedef struct { int match, mismatch, gap_open, gap_extend, min_score, tail; } vdjx_isotype_params;   /* 24 bytes */
int vdjx_constant_load(vdjx_ctx* ctx, const char* seqs, const uint64_t* off, size_t n);
int vdjx_isotype(vdjx_ctx* ctx, const char* contigs, size_t n, int len, const vdjx_isotype_params* params, vdjx_annot_hit* out_c,
                 int32_t* out_scores);

/* ---- D calls: the bases between the V and the J hit against the D segments ------------------------------------------------------------
 * gives `vdjer --airr` the d_call, the d_cigar and the N regions of a heavy-chain rearrangement (the part of the V-QUEST round trip that
 * vdjx_annotate left open).  All arithmetic is integer: the device's results are bitwise the model's (tests/dcall_model.py).
 *   D set       vdjx_dsegment_load: record r is seqs[off[r] .. off[r+1]), cleaned by the caller exactly as for vdjx_germline_load.  Every
 *               record given is a D record whatever its name (vdjx_germline_load still counts and skips class 'D': the caller hands the
 *               class-D records of the same FASTA to this call).  0 .. 4096 records of 1 .. 2047 bases.  The set lives in a device buffer
 *               of its own, independent of the germline and the constant set, until the next vdjx_dsegment_load or vdjx_shutdown.
 *   query       contig c's own window: contig[win_start[c] .. win_start[c] + win_len[c]), 0-based, given by the caller; win_len is
 *               0 .. VDJX_DCALL_WINDOW = 256 (a wave holds four window rows per lane); the window lies inside the contig.
 *   score       vdjx_annotate's recurrences and scoring rule, unchanged, window row i in 1..win_len[c], record r's column j in 1..g_r:
 *               S(contig, r) = max H (0 for an empty window).  out_scores (may be NULL) receives every S, out_scores[contig * C + r].
 *   call        the primary hit is the record of highest S, the lowest index on a tie; n_tied counts the records at that S and tied[]
 *               lists the first 8 of them in index order.  No call (gene -1, n_tied 0, tied[] -1) when S < min_score, when C = 0 or
 *               when win_len[c] = 0; score is S all the same.
 *   traceback   the primary hit only, by vdjx_annotate's rules and preference order; every field of vdjx_annot_hit means what it means
 *               there.  seq_start / seq_end are in CONTIG coordinates (window coordinate + win_start[c]); S = 0: no traceback.
 *   the window `vdjer --airr --d-calls` uses (d_window in vdjer_main.c, vdjer_amd/annot.py and the model): with a V hit and a J hit
 *               (gene >= 0 and score > 0, both), the bases strictly between them: start = v.seq_end, length = j.seq_start - 1 -
 *               v.seq_end; a length <= 0 (the hits abut or overlap) is length 0; a length > 256 is length 0 and counted; no V hit or
 *               no J hit is length 0.  A window of length 0 starts at 0.
 * Defaults (what `vdjer --d-calls` uses): match 2, mismatch 3, gap_open 5, gap_extend 2, min_score 22: eleven matched bases.  Against 34
 * random records of 11 .. 37 bases, 0.25 % of 400 random 24-base windows reach 22 (0.75 % reach 20; the highest S is 22), 0.5 % of 400
 * random 45-base windows (3.0 % reach 20; highest 26) and 0.75 % of 400 random 64-base windows (3.5 % reach 20; highest 23); 200 exact
 * cuts of 11 .. 16 bases, each planted in a random 45-base window, all score at least 22 and all are called for their own record
 * (tests/test_dcall_cpu.py measures these again).  It is a parameter of the model, not a tolerance.
 * NOT modelled: D genes in inverted orientation; a second D (D-D fusions); P nucleotides as distinct from N (np1 / np2 of the table are
 * whatever lies between the hits); IgBLAST's or V-QUEST's own D scoring.
 * VDJX_EINVAL: contigs of unequal length (a NUL inside the n*len characters), len >= 4096, n >= 2^20, match outside 1..15 or mismatch /
 * gap_open / gap_extend outside 0..31, min_score < 0, a negative win_start or win_len, win_len > 256, a window past the contig's end; more
 * than 4096 records or a record of 0 or >= 2048 bases (vdjx_dsegment_load).  vdjx_dcall before any vdjx_dsegment_load is VDJX_ESTATE.
 * n = 0 returns at once.  A call is three kernel dispatches (score, merge, trace) whatever n and C are.  Scratch comes from the context's
 * workspace; no floating point, no atomics: two calls give the same bits. */
#define VDJX_DCALL_WINDOW 256
typedef struct { int match, mismatch, gap_open, gap_extend, min_score; } vdjx_dcall_params;   /* 20 bytes */
int vdjx_dsegment_load(vdjx_ctx* ctx, const char* seqs, const uint64_t* off, size_t n);
int vdjx_dcall(vdjx_ctx* ctx, const char* contigs, size_t n, int len, const int32_t* win_start, const int32_t* win_len,
               const vdjx_dcall_params* params, vdjx_annot_hit* out_d, int32_t* out_scores);

/* ---- clonal lineages: single linkage over the junctions' length-normalised Hamming distance ---------------------------------------------
 * gives `vdjer --lineages` the clone_id of an AIRR rearrangement table: the grouping Change-O's DefineClones / SCOPer make of V'DJer's
 * output in a second tool (same V gene, same J gene, same junction length, single linkage on the nucleotide junctions).  All pairs of a
 * bucket are compared on the device.  All arithmetic is integer: the device's results are bitwise the model's (tests/lineage_model.py).
 *   items       item i is junctions[off[i] .. off[i+1]) of length L_i; group[i] is a key the caller chose (a V-gene / J-gene pair).  An
 *               item whose group is VDJX_LINEAGE_NONE takes no part: out_clone = -1, out_nearest = -1, any length, 0 included.
 *   bucket      the participating items of equal group and equal L.  They may lie anywhere in the input: nothing has to be sorted.
 *   distance    d(i, j) of two items of one bucket: the number of positions p in 0 .. L-1 at which the characters differ or either is not
 *               one of ACGT.  N never matches, not even N (as in vdjx_annotate); lower case is not ACGT.
 *   link        i and j are linked iff they share a bucket, i != j and d(i, j) * den <= num * L (exact: 255 * den fits 32 bits).
 *   clone       a connected component of the link graph (single linkage).  out_clone[i] is 0-based: the components are numbered in the
 *               order of their smallest member index.
 *   nearest     out_nearest[i] (may be NULL) = the smallest d(i, j) > 0 over the other items j of i's bucket, -1 when there is none (a
 *               bucket of one item, or of items all at distance 0): Change-O's distToNearest, left unnormalised.
 *   info        (may be NULL; zeroed first, every field filled on success) items: participating items; buckets; largest_bucket: the
 *               items of the largest; clones; pairs: the sum of m (m - 1) / 2 over the buckets of m items; links: unordered linked pairs.
 * Defaults (what `vdjer --lineages` uses): num / den = 1500 / 10000, the 0.15 SCOPer documents as a starting point.  It is a parameter of
 * the model, not a tolerance: out_nearest (the table's dist_nearest) is there so that a user can choose their own from its histogram, and
 * vdjx_lineage_threshold, below, chooses it from that histogram on the device.
 * NOT modelled: amino-acid distances (a 5-mer substitution distance: vdjx_lineage_model, below); N as a wildcard; clustering across
 * samples (complete and average linkage: vdjx_lineage_link, below); "first gene only" handling of tied V calls (the group is the caller's: `vdjer` keys on the whole
 * normalised tie list).
 * VDJX_EINVAL: n >= 2^20, a participating item of 0 or more than VDJX_LINEAGE_MAXLEN bases, offsets that decrease, den < 1, den > 10^6,
 * num < 0, num > den, NULL out_clone.  n = 0 returns at once with a zeroed info.  The (group, L, index) keys are sorted on the host (per
 * item); everything per pair runs on the device.  A call is five kernel dispatches (pack, pairs, flatten, number, out) whatever n and the
 * number of buckets are.  Scratch comes from the context's workspace; no floating point.  The union-find of the pair pass uses integer
 * atomics, and the larger root always goes under the smaller: the result does not depend on the order they land in, two calls give the
 * same bits.  Stats: "lineage_work_items" ((bucket, row block, column slice) items of the pair pass), "lineage_us" (host clock). */
#define VDJX_LINEAGE_NONE   0xFFFFFFFFu
#define VDJX_LINEAGE_MAXLEN 255
typedef struct { int num, den; } vdjx_lineage_params;                 /* 8 bytes  */
typedef struct { uint32_t items, buckets, largest_bucket, clones; uint64_t pairs, links; } vdjx_lineage_info;  /* 32 bytes */
int vdjx_lineage(vdjx_ctx* ctx, const char* junctions, const uint64_t* off, const uint32_t* group, size_t n,
                 const vdjx_lineage_params* params, int32_t* out_clone, int32_t* out_nearest, vdjx_lineage_info* info);

/* ---- clonal lineages under a 5-mer substitution distance (HH_S5F and its kin) ----------------------------------------------------------
 * gives `vdjer --lineages --lineage-model` what Change-O's DefineClones --model hh_s5f, shazam's distToNearest(model = "hh_s5f") and SCOPer
 * do with a targeting model: a mismatch is weighed by the 5-mer it happens in, so that a transition at a hot spot costs less than a rare
 * change in a cold context.  Every quantity is an integer except the table's construction on the host; the device's results are bitwise the
 * model's (tests/lineage_dist_model.py).
 *
 * vdjx_lineage_distance_table (plain C, no GPU, no context): the targeting weights -> the distance table.
 *   weight      uint32 [1024][4] as vdjx_selection takes it: row 256 a + 64 b + 16 c + 4 d + e of the 5-mer abcde (A 0, C 1, G 2, T 3), column
 *               the new base; the column of the centre base c is ignored.
 *   table       w' = max(w, 1) for the 3,072 off-centre cells; S = their sum (64 bits); d = -log10((double) w' / (double) S) (libm); mean =
 *               the sum of all d in index order (row by row, columns A C G T, centre skipped), added left to right in double, / 3072.0;
 *               t = floor(1000 * d / mean + 0.5), clamped to 1 .. 65535; a centre cell is 0.  shazam's calcTargetingDistance in thousandths:
 *               a mismatch under the uniform model costs exactly 1000.
 *   info        (may be NULL) mean, and the smallest and largest off-centre t.
 * VDJX_EINVAL: a NULL weight or table.
 *
 * vdjx_lineage_model: arguments, buckets, limits, refusals, clone numbering and info are vdjx_lineage's.
 *   distance    a, b of one bucket of length L.  At every position p where they differ or either character is not one of ACGT:
 *               side(a->b, p) = table[5-mer a[p-2 .. p+2]][b[p]] when 2 <= p <= L - 3, all five characters of a are ACGT and b[p] is ACGT,
 *               and 1000 otherwise; side(b->a, p) alike.  symmetry 0 ("avg", shazam's): the position costs side(a->b) + side(b->a);
 *               symmetry 1 ("min"): 2 * the smaller.  D(a, b) = the sum over these positions (at most 255 * 2 * 65535, fits 32 bits).  With
 *               a table of all 1000, D = 2000 * the Hamming distance of vdjx_lineage on every input; a junction of fewer than 5 bases has no
 *               5-mer and behaves so under any table.
 *   link        iff D * den <= 2000 * num * L: num / den is still a fraction of the length, now in units of a mean mismatch.
 *   nearest     the smallest D > 0 in the bucket, -1 when there is none (D = 0 iff the junctions are equal and all ACGT).
 * NOT modelled: shazam's NN padding with N-averaged 5-mers at the junction's ends (a position without a full ACGT 5-mer costs the mean);
 * amino-acid distances.  (Complete and average linkage: vdjx_lineage_link, below.  A threshold chosen automatically: vdjx_lineage_threshold, below, unit 2000.)
 * VDJX_EINVAL, beyond vdjx_lineage's: symmetry not 0 or 1, a NULL table, an off-centre cell of 0.  The host re-indexes the table to the packed
 * rows' code order; a call is five dispatches whatever n is (pack, k_lin_pairs_model, flatten, number, out).  The pair pass first takes the
 * Hamming count h of a pair: every counted position costs at least cmin = 2 * min(1000, smallest cell), so a pair with h * cmin past both the
 * bucket's dmax and the lane's smallest D so far gives neither a link nor a nearest and is not walked; no result depends on it.  No floating
 * point on the device, integer atomics only: two calls give the same bits.  Stats: vdjx_lineage's, "lineage_model_walked": the ordered
 * pairs (row, column) whose positions were walked, of 2 * info->pairs, and "lineage_model_positions": the positions those walks looked at
 * (two look-ups each where both sides have a 5-mer; a walk stops once its sum is past both dmax and the lane's smallest D). */
typedef struct { int num, den, symmetry; } vdjx_lineage_model_params;            /* 12 bytes */
typedef struct { double mean; uint32_t min_cost, max_cost; } vdjx_lineage_table_info;   /* 16 bytes */
int vdjx_lineage_distance_table(const uint32_t* weight /* [1024][4] */, uint16_t* table /* [1024][4] */, vdjx_lineage_table_info* info);
int vdjx_lineage_model(vdjx_ctx* ctx, const char* junctions, const uint64_t* off, const uint32_t* group, size_t n,
                       const vdjx_lineage_model_params* params, const uint16_t* table /* [1024][4] */, int32_t* out_clone,
                       int32_t* out_nearest, vdjx_lineage_info* info);

/* ---- clonal lineages under complete and average linkage ----------------------------------------------------------------------------------
 * gives `vdjer --lineages --lineage-link` what Change-O's DefineClones --link single|average|complete and SCOPer's hierarchicalClones(linkage =)
 * offer against the chaining of single linkage: two unrelated clones of one bucket no longer become one lineage through a run of
 * intermediates.  All arithmetic is integer; the device's results are bitwise the model's (tests/lineage_link_model.py).
 *   items, buckets, D(i, j), nearest   vdjx_lineage's (table NULL: D is the Hamming count d, unit = 1) or vdjx_lineage_model's (D the model's
 *               sum, unit = 2000; params->symmetry is looked at only then).  N never matches.  K = unit * num * L; a pair is linked iff
 *               D * den <= K.
 *   clusters    inside a bucket they start as the single items; a cluster's id is its smallest member index in the caller's order.  The
 *               dissimilarity of two clusters A, B is, under linkage 1 (complete), delta = max D(a, b) over a in A, b in B, and the pair is
 *               eligible iff delta * den <= K; under linkage 2 (average, UPGMA), S(A, B) = the sum of D(a, b), delta = S / (|A| |B|), eligible
 *               iff S * den <= K |A| |B|.  Among all eligible pairs with id(A) < id(B) the smallest under the strict order (delta, id(A),
 *               id(B)) is merged -- under average linkage delta is compared exactly, S1 n2 against S2 n1 --, the merged cluster keeps id(A),
 *               and this repeats until no pair is eligible.  The Lance-Williams updates are exact integers: max, and S(A u B, C) = S(A, C) +
 *               S(B, C).  Both linkages are reducible, so stopping at the threshold is cutting the dendrogram at it (cutree(h =),
 *               fcluster(criterion = 'distance')).  Where distances tie the partition depends on the caller's order of the items: the tie
 *               rule above is the definition.  Linkage 0 (single) returns bit for bit what vdjx_lineage (table NULL) or vdjx_lineage_model
 *               returns, and a zeroed link info.
 *   out_clone   the final clusters numbered in the order of their smallest member.
 *   info        the single-linkage pass': links and pairs keep their meaning; clones is the final number.
 *   link        (may be NULL; zeroed first) components: single-linkage components of two and more members; largest_component;
 *               merges; clones_single: the clones of linkage 0; batches; cells: matrix cells built (m * m for a component of m).
 * Two facts shape the implementation.  (1) Only linked components need agglomerating: a merge needs at least one linked cross pair (complete:
 * every cross pair is linked; average: the mean is at most the cut, so some pair is), so the final clusters refine the single-linkage
 * components and no merge ever crosses two of them.  The device agglomerates per component of the pair pass, never per bucket (the test
 * model agglomerates whole buckets).  (2) Everything fits 64 bits: a component has at most 4,096 members, so |A| |B| <= 2^22; K <= 2000 *
 * 10^6 * 255 < 2^39, so K |A| |B| < 2^61; eligibility is tested as S <= floor(K |A| |B| / den), the same predicate for an integer S with no
 * product of S and den; only eligible pairs are ever ordered, and for them S <= 510,000 * 2^22 < 2^41, so S1 n2 < 2^63.
 * The device: the members of the components of two and more are laid out in component order (components by their smallest member, members by
 * index; on the host from the flattened roots, per item) and go in batches of whole components of at most VDJX_LINK_CELLS matrix cells
 * (default 2^26, 1 .. 2^28, read per call; a component of more cells goes alone; any value gives the same bytes).  Per batch k_link_matrix
 * (k_link_matrix_model under a table) builds every component's full matrix and k_link_merge agglomerates a component per workgroup, with a
 * cached best partner per cluster, so that a merge costs the row update and the repair of the caches that pointed at A or B; components of
 * up to 88 members keep their matrix in LDS.  No floating point, no atomic whose order shows: two calls give the same bits.
 * VDJX_EINVAL: what vdjx_lineage refuses, with a table what vdjx_lineage_model refuses, a linkage outside 0 .. 2.  VDJX_ELIMIT: under linkage
 * 1 or 2 a single-linkage component of more than 4,096 members (the message names its size); single linkage has no such limit.
 * NOT modelled: Ward or median linkage; a dendrogram as output; a threshold per bucket.
 * Stats: vdjx_lineage's (and vdjx_lineage_model's), "lineage_link_us" (host clock from the roots to the last launch), "lineage_link_cells". */
typedef struct { int num, den, symmetry, linkage; } vdjx_lineage_link_params;   /* 16 bytes */
typedef struct { uint32_t components, largest_component, merges, clones_single, batches, reserved; uint64_t cells; } vdjx_lineage_link_info;  /* 32 bytes */
int vdjx_lineage_link(vdjx_ctx* ctx, const char* junctions, const uint64_t* off, const uint32_t* group, size_t n,
                      const vdjx_lineage_link_params* params, const uint16_t* table /* [1024][4]; NULL: Hamming */, int32_t* out_clone,
                      int32_t* out_nearest, vdjx_lineage_info* info, vdjx_lineage_link_info* link);

/* ---- the lineage threshold: the valley between the two modes of the nearest-neighbour distances ----------------------------------------
 * gives `vdjer --lineages --lineage-threshold` what shazam's findThreshold(method = "density") makes of distToNearest before DefineClones
 * runs: the distances to the nearest neighbour have a mode of clonal relatives and a mode of unrelated sequences, and the threshold is the
 * valley between them.  Everything is integer except the construction of the kernel tables on the host: the device's results are bitwise
 * the model's (tests/threshold_model.py).
 *   constants   G = 10,000: the grid is g = 0 .. G, G + 1 points of 0.0001, the unit of --lineage-dist.  FIX = 2^30.
 *   inputs      nearest[n]: out_nearest of the two lineage calls, -1: none; length[n]: the junctions' lengths; unit: 1 for vdjx_lineage's
 *               distances, 2000 for vdjx_lineage_model's.
 *   bins        an item with nearest < 0 takes no part and its length is not read.  Any other falls into bin v = min(G, (2 G nearest +
 *               unit L) / (2 unit L)) by 64-bit integer division: nearest / (unit L) rounded half up to the grid, clamped at 1.0.  c[v]
 *               counts the items of bin v; values = the sum of c, distinct = the bins that are not 0.
 *   tables      vdjx_threshold_kernel (plain C, no GPU, no context), k = 1 .. VDJX_THRESHOLD_MAX_K: w[d] = floor(FIX * exp(-(double)(d * d) /
 *               (double)(200 * k * k)) + 0.5) with libm's exp, for d = 0, 1, .. up to the first d that gives 0; every entry from there on is 0
 *               (the table does not increase).  *len (may be NULL) = the entries before it.  A Gaussian with a standard deviation of 10 k grid
 *               steps, the bandwidth h = k / 1000; w[0] = FIX; len is about 65.6 k, so from k = 153 on the table covers the whole grid.
 *   density     Y_k[g] = the sum over v of c[v] * w_k[|g - v|], in uint64 (values < 2^20: Y < 2^50).
 *   peaks       of row k: cut 0 .. G into maximal runs of equal Y.  A run is a peak when its Y > 0, is greater than the run before it (or
 *               there is none) and greater than the run after it (or there is none).  A peak is counted when Y << peak_shift >= the row's
 *               largest Y: a bump below 1 / 2^peak_shift of the highest peak, an outlier in the far tail, is ignored.  peaks_all[k] and
 *               peaks[k] are the two counts.
 *   bandwidth   k* = the smallest k in 1 .. max_k with peaks[k] <= 2: Silverman's critical bandwidth for two modes, over a fixed list.
 *   valley      with two counted peaks: a = the last point of the first peak's run, b = the first point of the second's; m = the smallest Y
 *               over a < g < b; t_first, t_last = the first and last g there with Y = m; threshold = (t_first + t_last) / 2 rounded down,
 *               the middle of the valley's floor (which matters when the floor is a run of zeros).  The valley is accepted when valley_den *
 *               m <= valley_num * min(Y_a, Y_b).
 *   status      VDJX_THRESHOLD_FOUND; _FEW: fewer than min_values values, no density is computed; _NO_SCALE: no k up to max_k with at most two
 *               counted peaks; _ONE_MODE: one counted peak at k*; _SHALLOW: two peaks and a valley the guard refuses.  With any status but
 *               FOUND the threshold is 0 and the caller keeps its own.
 *   outputs     (each of the three may be NULL) out_hist[G + 1]: c; out_density[G + 1]: row k*, row max_k under _NO_SCALE, zeros under _FEW;
 *               out_peaks[max_k][2]: peaks_all and peaks of every row (zeros under _FEW).
 *   info        (zeroed first) values, distinct, status; k: k*, max_k under _NO_SCALE, 0 under _FEW; of that row peaks_all, peaks, ymax, the
 *               first counted peak's first and last point and Y (p1_first, p1_last, y1) and, with two or more, the second's; with exactly two
 *               (FOUND, _SHALLOW) t_first, t_last, m; threshold.
 * Defaults (what `vdjer --lineage-threshold` uses): max_k 200, peak_shift 5, valley 1 / 2, min_values 10.
 * NOT modelled: shazam's "gmm" method; its bandwidth selector (this is the critical bandwidth over thousandths); subsampling (the
 * distances are exact and all there); a threshold per V/J bucket; a confidence interval of the threshold.
 * VDJX_EINVAL: n >= 2^20, nearest < -1, a participating length of 0 or above 255, unit 0 or above 2^20, max_k outside 1 .. 200, peak_shift
 * outside 0 .. 13, valley_den < 1 or > 10^6, valley_num outside 0 .. valley_den, min_values < 1, a NULL info; vdjx_threshold_kernel: k
 * outside 1 .. 200, a NULL w.  n = 0 is status _FEW.
 * A call is five kernel dispatches whatever n is (histogram, number, compact, density, peaks; the histogram alone under _FEW, none without a
 * value).  The items are counted in LDS histograms with integer atomics; the non-zero bins are compacted to an ascending list; the density
 * pass is a grid of (tiles of VDJX_THRESHOLD_TILE grid points, k) with w_k in LDS; a workgroup per k finds the row's peaks.  The host picks
 * k* from the max_k records and reads that one row back for the valley: the max_k x (G + 1) matrix stays on the device.  The tables are
 * built once per process on the host (about 1.2 M exp, 5 MB) and their leading non-zero entries uploaded per call.  Scratch comes from the
 * context's workspace; no floating point on the device, integer atomics only: two calls give the same bits.  Stats: "threshold_us" (host
 * clock), "threshold_macs" (the terms c[v] * w_k[|g - v|] with |g - v| < len_k, all k), "threshold_table_us" (the tables' one build). */
#define VDJX_THRESHOLD_GRID  10000u
#define VDJX_THRESHOLD_MAX_K 200
#define VDJX_THRESHOLD_TILE  256u       /* grid points per workgroup of the density pass (the tests place modes on a tile's ends) */
#define VDJX_THRESHOLD_FOUND    0u
#define VDJX_THRESHOLD_FEW      1u
#define VDJX_THRESHOLD_NO_SCALE 2u
#define VDJX_THRESHOLD_ONE_MODE 3u
#define VDJX_THRESHOLD_SHALLOW  4u
typedef struct { int max_k, peak_shift, valley_num, valley_den, min_values; } vdjx_threshold_params;     /* 20 bytes */
typedef struct { uint32_t values, distinct, status, k, peaks_all, peaks, p1_first, p1_last, p2_first, p2_last, t_first, t_last, threshold, reserved;
                 uint64_t y1, y2, m, ymax; } vdjx_threshold_info;                                          /* 88 bytes */
int vdjx_threshold_kernel(int k, uint32_t* w /* [G + 1] */, uint32_t* len);
int vdjx_lineage_threshold(vdjx_ctx* ctx, const int32_t* nearest, const uint32_t* length, size_t n, uint32_t unit,
                           const vdjx_threshold_params* params, uint32_t* out_hist /* [G + 1] */, uint64_t* out_density /* [G + 1] */,
                           uint32_t* out_peaks /* [max_k][2] */, vdjx_threshold_info* info);

/* ---- lineage trees: the minimum spanning tree of every clone under the Hamming distance of its members' common window -------------------
 * gives `vdjer --trees` what a repertoire user looks at inside a lineage (alakazam / dowser / Change-O BuildTrees): which member is
 * closest to the germline, who descends from whom, how many mutations apart.  All pairs of a clone are compared on the device, over the
 * whole window and not the junction alone.  All arithmetic is integer: the device's results are bitwise the model's (tests/tree_model.py).
 *   items       contig i is contigs[i*len .. (i+1)*len).  clone[i] is any key >= 0 (typically out_clone of the lineage call above); an
 *               item with clone[i] = -1 takes no part: out_parent = out_dist = out_depth = -1.  The members of a clone may lie anywhere
 *               in the input: nothing has to be sorted.
 *   window      anchor[i] in 0 .. len: where the junction starts in contig i.  The members of a clone are compared over their common
 *               window around the anchor: with a = min anchor and b = min (len - anchor) over the clone's members, contig i contributes
 *               contig_i[anchor[i] - a .. anchor[i] + b), w = a + b bases.  The shift between two members is arbitrary.
 *   distance    d(i, j) of two members of one clone: the number of window positions at which the characters differ or either is not
 *               one of ACGT: the rule of the lineage call (N never matches, not even N; lower case is not ACGT).
 *   tree        the minimum spanning tree of the complete graph on a clone's members under the strict order of the keys
 *               (d(i, j), min(i, j), max(i, j)), the indices the caller's.  The order is total: the tree is unique, and Boruvka's
 *               rounds (every component takes the smallest edge that leaves it) cannot close a cycle.
 *   root        the member with the smallest (prio[i], i); prio = NULL: the smallest index.  out_parent[i] is the next item on the tree
 *               path to the root (-1 for the root), out_dist[i] = d(i, parent) (-1 for the root), out_depth[i] the edges to the root.
 *   info        (may be NULL; zeroed first, every field filled on success) members: participating items; clones; largest_clone: the
 *               members of the largest; edges = members - clones; weight: the sum of every out_dist >= 0; rounds = ceil(log2
 *               largest_clone), the Boruvka passes launched: 0 when no clone has two members.
 * NOT modelled: alignment of members that differ by an indel (the comparison is column by column); maximum parsimony or likelihood; a
 * germline sequence as a node of its own: the root is an observed contig.  Inferred intermediate nodes and Newick output: vdjx_tree_nj; a
 * search for the tree of fewest mutations: vdjx_tree_mp.
 * VDJX_EINVAL: n >= 2^20, len < 1 or len >= 4096, contigs of unequal length (a NUL inside the n*len characters), clone[i] < -1, a member's
 * anchor outside 0 .. len, an empty window (w = 0: a member anchored at 0 and one at len), NULL out_parent / out_dist / out_depth.  n = 0
 * returns at once with a zeroed info.  The (clone, index) keys are sorted on the host (per item), which also computes the windows;
 * everything per pair runs on the device: a call is 1 + 3 * rounds kernel dispatches (pack; per round min, hook, flat) whatever n and the
 * number of clones are, and nothing is read back between the rounds.  The edges come back once; orienting them toward the roots and
 * counting the depths is O(n) on the host.  Scratch comes from the context's workspace; no floating point.  Integer atomics are a
 * minimum per component, the union-find of the lineage call and the slot of an appended edge, none of which the outputs depend on the
 * order of: two calls give the same bits.  Stats: "tree_work_items" ((clone, row block, column slice) items of a round), "tree_rounds",
 * "tree_us" (host clock). */
typedef struct { uint32_t members, clones, largest_clone, rounds; uint64_t edges, weight; } vdjx_tree_info;   /* 32 bytes */
int vdjx_tree(vdjx_ctx* ctx, const char* contigs, size_t n, int len, const int32_t* clone, const int32_t* anchor, const uint32_t* prio,
              int32_t* out_parent, int32_t* out_dist, int32_t* out_depth, vdjx_tree_info* info);

/* ---- edge support for the lineage trees: the delete-half jackknife over the window's columns ------------------------------------------
 * the tree above is unique, so it looks equally certain everywhere, though many of its edges are decided by one or two columns.  Every
 * replicate keeps each window column with probability 1/2 and builds the trees again on the kept columns alone; an edge's support is
 * the number of replicates whose tree still has it (Felsenstein's delete-half jackknife: deleting columns keeps the distance a popcount).
 * All arithmetic is integer: the device's results are bitwise the model's (tests/tree_support_model.py).
 *   items       contigs, n, len, clone[], anchor[] exactly as vdjx_tree takes them; the windows and (a, b) are as there.  Window position
 *               q = 0 is the character at anchor[i] - a.
 *   parent      parent[i]: for a member, the item whose edge to it is to be scored, or -1 (typically out_parent of vdjx_tree; it need not
 *               be a minimum spanning tree).
 *   keep rule   mix64(x) is splitmix64's output step in 64-bit wrap-around arithmetic: z = x + 0x9E3779B97F4A7C15;
 *               z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) * 0x94D049BB133111EB; the result z ^ z >> 31
 *               (mix64(0) = 0xE220A8397B1DCDAF).  Replicate r (1 .. replicates) keeps window position q when bit q & 31 of
 *               mix64(seed ^ ((uint64_t) r << 32 | q >> 5)) is set: the rule depends on (seed, r, q) only, the same for every clone.
 *   replicate   d_r(i, j): the number of KEPT window positions at which the two members differ or either is not one of ACGT.  The
 *               replicate tree of a clone is the minimum spanning tree under the strict order of the keys (d_r, min(i, j), max(i, j)),
 *               unique as above.  A replicate that keeps no position of a clone's window has all distances 0: the star at the
 *               smallest index.
 *   output      out_support[i], for a member with parent[i] >= 0: the number of replicates whose tree contains the undirected edge
 *               {i, parent[i]}; -1 for every other item.
 *   info        (may be NULL; zeroed first, every field filled on success) members, clones, largest_clone as vdjx_tree's; replicates;
 *               batches: the groups of whole replicates the device ran side by side (0 when no clone has two members); rounds =
 *               ceil(log2 largest_clone), Boruvka's rounds per batch; edges: the parent[i] >= 0; matched: the sum of the supports; full:
 *               the edges with support = replicates.
 * NOT modelled: the bootstrap with replacement (support of splits -- bipartitions -- rather than of edges, for the trees with inferred
 * nodes: vdjx_tree_split_support).  An edge whose only differing
 * columns are all deleted can still appear in a replicate through the index tie-break, so for such edges the support is an upper bound
 * (a 12-member descent with dist_parent = 1 everywhere gave supports between 5/16 and 16/16: informative, not exact).
 * VDJX_EINVAL: everything vdjx_tree refuses; replicates outside 1 .. 1024; a parent[i] that is i, outside -1 .. n-1 or in another clone;
 * a parent[i] >= 0 on an item with clone[i] = -1; NULL parent or out_support.  n = 0 returns at once with a zeroed info.
 * The host computes every replicate's ascending list of kept positions; a batch is max(1, floor(R / members of clones of two and more))
 * whole replicates laid side by side (the edge keys carry row numbers below 2^20; R = VDJX_TREE_SUPPORT_ROWS, 1 .. 2^20 - 1, the
 * default 2^20 - 1) and 1 + 3 * rounds + 1 dispatches (pack, the rounds of vdjx_tree, count) whatever n, the clones and the replicates
 * in it are.  Per batch only the edge count is read back, the supports once at the end.  The count is an integer atomicAdd per edge:
 * two calls give the same bits.  Stats: "tree_support_batches", "tree_support_work_items" (the work items of a round, summed over the
 * batches), "tree_support_us" (host clock). */
typedef struct { uint32_t replicates; uint64_t seed; } vdjx_tree_support_params;                                /* 16 bytes */
typedef struct { uint32_t members, clones, largest_clone, replicates, batches, rounds; uint64_t edges, matched, full; } vdjx_tree_support_info;   /* 48 bytes */
int vdjx_tree_support(vdjx_ctx* ctx, const char* contigs, size_t n, int len, const int32_t* clone, const int32_t* anchor,
                      const int32_t* parent, const vdjx_tree_support_params* params, int32_t* out_support, vdjx_tree_support_info* info);

/* ---- neighbour-joining lineage trees with inferred ancestors ---------------------------------------------------------------------------
 * a minimum spanning tree can only hang observed contigs under observed contigs: two sisters that share three mutations become parent and
 * child, and the ancestor that carried the three is nowhere.  This call gives `vdjer --trees-nj` what alakazam's buildPhylipLineage and
 * dowser's getTrees add to a clone table: the unobserved ancestors, branch lengths between them, and (through the command line) a Newick
 * file.  All arithmetic is integer: the device's results are bitwise the model's (tests/tree_nj_model.py).
 *   items       contigs, n, len, clone[], anchor[], prio exactly as vdjx_tree takes them; the windows (a, b), w = a + b and the distance
 *               d(i, j) are as there.
 *   nodes       inside a lineage of m members the leaves have ids 0 .. m - 1 in ascending caller index; inferred nodes get m, m + 1, ...
 *               in the order they are made: max(0, m - 2) of them, and for m >= 2 there are 2m - 3 edges.
 *   joining     D[i][j] = d(i, j) << 16 (64-bit).  While more than three nodes are active, r of them: R[i] = the sum of D[i][k] over
 *               the active k != i; Q(i, j) = (r - 2) D[i][j] - R[i] - R[j]; the pair with the smallest key (Q, i, j), i < j by node id,
 *               is joined into a new node u with b_i = floor(((r - 2) D[i][j] + R[i] - R[j]) / (2 (r - 2))) (toward minus infinity),
 *               b_j = D[i][j] - b_i and D[u][k] = floor((D[i][k] + D[j][k] - D[i][j]) / 2) for every other active k.  The last three
 *               x < y < z meet in one more node: b_x = floor((D[x][y] + D[x][z] - D[y][z]) / 2), b_y = D[x][y] - b_x, b_z = D[x][z] -
 *               b_x.  m = 3 is that step alone, m = 2 the one edge of length D[0][1], m = 1 a lone root.  Negative branch lengths are
 *               kept as computed (as ape's nj does) and counted.  Where distances tie the tree depends on the order of the contigs: the
 *               key is the definition.
 *   root        the member with the smallest (prio[i], i), as vdjx_tree's; that leaf is the root of its lineage's tree and its single
 *               neighbour its only child, so every inferred node has exactly two children.
 *   ancestors   Fitch parsimony, every window column on its own, the base order A < C < G < T.  A leaf's set is its base if that is one
 *               of ACGT, else all four: a character that never matches in the distance is a wildcard here, so an N costs branch length
 *               but never a mutation.  Upward an inferred node's set is the intersection of its children's sets if that is not empty,
 *               else their union.  The root's set is its leaf set intersected with its child's set if that is not empty, else its leaf
 *               set; its state the lowest base of it.  Downward a node's state is its parent's state if that lies in its set, else the
 *               lowest base of its set -- leaves too: a wildcard leaf takes its parent's base.  An inferred node's sequence is its w
 *               states; a node's mutations the window columns at which its state differs from its parent's.
 *   outputs     [nodes] each, nodes = vdjx_tree_nj_nodes(clone, n) = n + the sum of max(0, m - 2).  Slots 0 .. n - 1 are the caller's
 *               items; the inferred nodes follow from slot n, lineage after lineage in ascending clone key, in creation order inside a
 *               lineage.  out_parent holds slots; out_length the edge to the parent in 1/65536; out_depth the edges to the root;
 *               out_clone the lineage's key.  A root has parent -1, length 0 and mutations -1; an item with clone = -1 has -1
 *               everywhere.  out_anc (may be NULL: the mutations are still counted) is [nodes - n][len]: the inferred node's w states
 *               as characters, NUL from w on.
 *   info        (may be NULL; zeroed first, every field filled on success) members, clones, largest_clone as vdjx_tree's; internal: the
 *               inferred nodes; batches; negative: the edges of negative length; edges; joins: the pair joins, the sum of max(0, m - 3);
 *               cells: the sum of m * m over the lineages of two and more; parsimony: the sum of the mutations; length: of the lengths.
 * NOT modelled: maximum likelihood; dnapars' search over topologies (vdjx_tree_mp searches by nearest-neighbour interchanges from this
 * tree); the germline as a node of its own; alignment of members that differ
 * by an indel; Sankoff costs from a targeting model (they are vdjx_tree_sankoff's, below).  Support values for this tree:
 * vdjx_tree_split_support.
 * VDJX_EINVAL: everything vdjx_tree refuses, and a NULL output other than out_anc.  VDJX_ELIMIT: a lineage of more than
 * VDJX_NJ_MAX_MEMBERS members, named with its size before any GPU work.  n = 0 returns at once with a zeroed info.
 * The host sorts the keys and computes the windows as vdjx_tree does.  The lineages of two and more run in batches of whole lineages of at
 * most VDJX_NJ_CELLS matrix cells of 8 bytes (1 .. 2^28, the default 2^26, read per call; a lineage of more cells goes alone; any value
 * gives the same bytes).  A batch is the matrix kernel (a wave per lineage, row block and column slice, storing d << 16), the join kernel
 * (a workgroup per lineage: the matrix in LDS up to VDJX_NJ_LDS_MEMBERS members -- 32 KiB, four workgroups per CU -- and in global memory
 * beyond; a fixed m - 3 rounds of a block-wide arg-min in 64-bit integers and a row update, m^3 / 6 evaluations of Q in all) and, after
 * the host has rooted the edges (O(nodes)), Fitch's two passes (a wave per lineage and 64 columns, a lane per column).  Integer atomics
 * are sums only: two calls give the same bits.  No floating point; scratch comes from the context's workspace.  Stats: "tree_nj_us" (host
 * clock), "tree_nj_cells", "tree_nj_joins". */
#define VDJX_NJ_LDS_MEMBERS  64u        /* the largest lineage whose matrix the join kernel keeps in LDS (the tests run this size and the next) */
#define VDJX_NJ_MAX_MEMBERS  4096u
typedef struct { uint32_t members, clones, largest_clone, internal, batches, negative;
                 uint64_t edges, joins, cells, parsimony; int64_t length; } vdjx_tree_nj_info;                  /* 64 bytes */
int vdjx_tree_nj_nodes(const int32_t* clone, size_t n, uint64_t* nodes);      /* plain C, no GPU: n + the sum of max(0, m - 2) */
int vdjx_tree_nj(vdjx_ctx* ctx, const char* contigs, size_t n, int len, const int32_t* clone, const int32_t* anchor, const uint32_t* prio,
                 int32_t* out_parent, int64_t* out_length, int32_t* out_mutations, int32_t* out_depth, int32_t* out_clone /* each [nodes] */,
                 char* out_anc /* [nodes - n][len], NUL past w; may be NULL */, vdjx_tree_nj_info* info);

/* ---- maximum-parsimony lineage trees by a search over nearest-neighbour interchanges ---------------------------------------------------
 * vdjx_tree_nj prints Fitch's parsimony of a tree nobody tried to make parsimonious.  alakazam's buildPhylipLineage runs dnapars and
 * dowser's getTrees defaults to pratchet: both search over topologies for the tree of fewest mutations.  This call gives `vdjer
 * --trees-mp` a hill-climbing search of that kind.  It is integer throughout: the device's results are bitwise the model's
 * (tests/tree_mp_model.py).
 *   items       contigs, n, len, clone[], anchor[], prio, the windows, the root and the node ids exactly as vdjx_tree_nj's: a lineage of m
 *               members has the leaves 0 .. m - 1 in ascending caller index and the inferred nodes m .. 2m - 3; the root is the leaf of
 *               smallest (prio, index) and its single neighbour its only child; every inferred node has two children, kept ascending by
 *               local id.  The output slots are vdjx_tree_nj's: the items first, the inferred nodes from slot n, lineage after lineage in
 *               ascending clone key.
 *   start       start_parent[nodes], in those slots, is the caller's topology; only the entries of lineage members other than the roots
 *               and of inferred nodes are read.  NULL: the tree vdjx_tree_nj gives the same arguments (that function's own steps are run as far
 *               as its parents: its bits are the contract).  The ids of the inferred nodes are the start's and never change.
 *   score       P(T): the sum over the window columns of Fitch's union events.  A leaf's set is its base if that is one of ACGT, else all
 *               four (vdjx_tree_nj's wildcard rule); an inferred node's set is the intersection of its children's sets if that is not
 *               empty, otherwise their union, and the column costs 1; at the root the column costs 1 more if the root leaf's set and its
 *               child's set do not meet.  P(T) equals the sum of the edge mutations of vdjx_tree_nj's two passes on T, wildcards included.
 *   candidates  (v, k): an inferred node v whose parent p is an inferred node too, k in {0, 1}.  With s p's other child and c = kid[v][k]
 *               (ascending), the candidate swaps s and c: afterwards v's children are {s, kid[v][1 - k]} and p's {c, v}, both ascending
 *               again, and the parents of s and c are exchanged.  A lineage of m members has 2 (m - 3); m <= 3 is not searched.
 *   round       one round of one lineage scores every candidate; the one of smallest key (P, v, k) is applied if its P is below the
 *               current P, otherwise the lineage is finished.  Where scores tie the key is the definition: the tree depends on the order
 *               of the contigs.  params.max_rounds caps the scoring rounds of a lineage (0: until it is finished; every move lowers P by at
 *               least 1, so the search ends on its own).
 *   finish      Fitch's two passes on the final topology, exactly vdjx_tree_nj's rules: every inferred node's sequence, every node's
 *               mutations and depth.  There are no separate branch lengths: an edge's length is its mutations.
 *   outputs     [nodes] each, nodes = vdjx_tree_nj_nodes(clone, n); out_parent holds slots; a root has parent -1, depth 0, mutations -1;
 *               an item with clone = -1 has -1 everywhere.  out_anc (may be NULL) is [nodes - n][len], NUL from w on.
 *   info        (may be NULL; zeroed first) members, clones, largest_clone, internal, edges, batches as vdjx_tree_nj's; searched: the
 *               lineages of four and more members; moved: those with at least one move; moves; rounds: the most scoring rounds any lineage
 *               had; candidates: the sum over the lineages and their scoring rounds of 2 (m - 3); parsimony_start: P of the start trees;
 *               parsimony: the sum of the final mutations (= P of the final trees).
 * NOT modelled: subtree pruning and regrafting, the rearrangement of dnapars and pratchet (it is vdjx_tree_spr's, below); TBR and random
 * restarts (modelled nowhere).  Nearest-neighbour interchanges stop in local optima, and from a poor start -- a caterpillar -- the search
 * ends far above what it reaches from vdjx_tree_nj's tree.  Collapsing zero-length edges into multifurcations; a germline node; Sankoff
 * costs (vdjx_tree_sankoff, below, is this search under a cost matrix).  Support values: vdjx_tree_split_support (its replicates are
 * neighbour-joining trees, not searched ones).
 * VDJX_EINVAL: everything vdjx_tree_nj refuses; params->reserved != 0; a start_parent that is no such tree -- a parent outside the
 * lineage, a root leaf without exactly one child, an inferred node without exactly two, another leaf with children, a cycle -- named with
 * the lineage's clone key, before any GPU work.  VDJX_ELIMIT: a lineage of more than VDJX_MP_MAX_MEMBERS members, named with its size
 * before any GPU work.  n = 0 returns at once with a zeroed info.
 * Batches are vdjx_tree_nj's (whole lineages under VDJX_NJ_CELLS; any value gives the same bytes).  A batch keeps kid, par, one set byte
 * per (inferred node, column), P and one int32 per candidate on the device.  A round is two dispatches: the scorer (a wave per lineage
 * and candidate, 64 columns at a time; a swap at (v, k) changes only the sets of v, p and p's ancestors, so a lane recomputes those two and walks
 * towards the root against the stored sets of the other children, until a wave-wide ballot says that no lane's set changed; integer
 * atomicAdd of the wave's sum) and pick-and-apply (a workgroup per lineage still searching: block-wide arg-min of (delta, v, k), one thread
 * rewires, all rewrite the stored sets along the path).  The host reads one counter per round from page-locked memory.  Then the host
 * roots the final kid / par and vdjx_tree_nj's Fitch kernel runs unchanged.  Integer atomics are sums only: two calls give the same bits.
 * No floating point; scratch comes from the context's workspace.  Stats: "tree_mp_us" (host clock over "tree_nj_us"'s span, from after the
 * argument checks: the key sort, the layout and the start tree included),
 * "tree_mp_candidates" (candidates scored), "tree_mp_steps" (the node updates the scorer made, counted per candidate and column tile: it
 * depends on the launch geometry, so it is a stat and no info field; full rescoring would make candidates x (m - 2) per tile). */
#define VDJX_MP_MAX_MEMBERS VDJX_NJ_MAX_MEMBERS
typedef struct { uint32_t max_rounds, reserved; } vdjx_tree_mp_params;          /* reserved must be 0 */
typedef struct { uint32_t members, clones, largest_clone, internal, batches, searched, moved, rounds;
                 uint64_t edges, moves, candidates, parsimony_start, parsimony; } vdjx_tree_mp_info;           /* 72 bytes */
int vdjx_tree_mp(vdjx_ctx* ctx, const char* contigs, size_t n, int len, const int32_t* clone, const int32_t* anchor, const uint32_t* prio,
                 const int32_t* start_parent /* [nodes] or NULL */, const vdjx_tree_mp_params* params /* NULL: {0, 0} */,
                 int32_t* out_parent, int32_t* out_mutations, int32_t* out_depth, int32_t* out_clone /* each [nodes] */,
                 char* out_anc /* [nodes - n][len]; may be NULL */, vdjx_tree_mp_info* info);

/* ---- maximum-parsimony lineage trees by a search over subtree prunings and regraftings (SPR) --------------------------------------------
 * vdjx_tree_mp rearranges by nearest-neighbour interchanges only and stops in their local optima.  dnapars (alakazam's buildPhylipLineage)
 * and pratchet (dowser's getTrees) both prune a subtree and regraft it anywhere else in the tree.  This call is vdjx_tree_mp with that
 * neighbourhood.  It is integer throughout: the device's results are bitwise the model's (tests/tree_spr_model.py).  There is no `vdjer`
 * flag for it yet: the call is reached through this header and vdjer_amd.api.
 *   items, start, score, finish, outputs   exactly vdjx_tree_mp's: contigs, n, len, clone[], anchor[], prio, the windows, the leaf sets with
 *               a wildcard for anything that is not ACGT, the local ids (leaves 0 .. m - 1, inferred nodes m .. 2m - 3), the root leaf r of
 *               smallest (prio, index) with its only child, children kept ascending, the output slots, start_parent[nodes] or NULL for
 *               vdjx_tree_nj's tree, P(T), Fitch's two passes on the final topology.  The ids of the inferred nodes never change.
 *   candidates  a lineage of m >= 4 members is searched.  A candidate is (c, y).  c, the pruned node, is any node other than r and r's
 *               child.  With p = parent(c), s p's other child and g = parent(p), T' is the tree without the subtree of c and with p
 *               dissolved: s takes p's place under g (and is r's child if g = r).  y is the lower end of an edge of T': any node of T'
 *               other than r and other than s -- the edge above s is the old place.  One c has 2 (m - leaves(c)) - 4 candidates; at m = 4
 *               these are the nearest-neighbour interchanges.
 *   apply       with x = parent(y) in T': s replaces p among g's children; p replaces y among x's children (p becomes r's child if x = r);
 *               p's children become {c, y}; every pair of children is sorted ascending again.  r never moves.
 *   round       one round of one lineage scores every candidate; the one of smallest key (P, c, y) is applied if its P is below the
 *               current P, otherwise the lineage is finished.  Where scores tie the key is the definition: the tree depends on the order
 *               of the contigs (as vdjx_tree_mp's, vdjx_tree_nj's and vdjx_lineage_link's results do).  params.max_rounds caps the scoring
 *               rounds of a lineage (0: until it is finished; every move lowers P by at least 1, so the search ends on its own).
 *   info        (may be NULL; zeroed first) the fields and meanings of vdjx_tree_mp_info, but candidates: the sum over the lineages and
 *               their scoring rounds of that round's candidates, which depend on the tree.
 * NOT modelled: TBR, which also re-roots the pruned subtree; random restarts and the parsimony ratchet; collapsing zero-length edges into
 * multifurcations; a germline node; Sankoff costs (vdjx_tree_sankoff, below, has them for the interchange search, vdjx_tree_sankoff_spr for this one); a
 * search per jackknife replicate (vdjx_tree_split_support's replicates are
 * neighbour-joining trees).  A steepest descent is not guaranteed to end below vdjx_tree_mp's tree on every input.
 * VDJX_EINVAL: everything vdjx_tree_mp refuses, with the same messages under this function's name.  VDJX_ELIMIT: a lineage of more than
 * VDJX_SPR_MAX_MEMBERS members, named with its clone key and size before any GPU work (the limit is the search's, so it is never met
 * below four members).  n = 0 returns at once with a zeroed info.
 * Batches are vdjx_tree_nj's (whole lineages under VDJX_NJ_CELLS; any value gives the same bytes).  A batch keeps kid, par, the root's
 * child, one up set per (inferred node, column), P and one 64-bit key per node on the device.  Fitch's length of an unrooted tree does
 * not depend on the root, so P(T after (c, y)) = P(T') + P(subtree c) + #{columns: comb(U'(y), D'(y)) and U(c) do not meet}: U' are the up
 * sets of T', which differ from the stored ones only on the path from g to r, and D' the down sets, D'(r's child) = r's set, D'(y) =
 * comb(D'(x), U'(y's sibling)).  The first two terms less P(T) are the same for every y: minus p's union event, plus the changes on that
 * path and at the root step.  A round is the scorer (a wave per lineage and pruned node, 64 columns at a time: the path walk, then one
 * pre-order walk of T' that yields every edge's score; a byte per (node, lane) in LDS up to 128 members, in the workspace beyond;
 * O(m^2 w) per lineage and round) and pick-and-apply (a workgroup per lineage still searching: arg-min of (delta, c, y), one thread
 * rewires, all rewrite the stored sets along the two changed paths).  The host reads one counter per round from page-locked memory, roots
 * the final kid / par, and vdjx_tree_nj's Fitch kernel runs unchanged; the search's P must equal the sum of the final mutations
 * (VDJX_ESTATE otherwise).  Integer atomics are sums only: two calls give the same bits.  No floating point; scratch comes from the
 * context's workspace.  Stats: "tree_spr_us" (host clock over "tree_mp_us"'s span), "tree_spr_candidates". */
#define VDJX_SPR_MAX_MEMBERS 1024u
typedef struct { uint32_t max_rounds, reserved; } vdjx_tree_spr_params;         /* reserved must be 0 */
typedef struct { uint32_t members, clones, largest_clone, internal, batches, searched, moved, rounds;
                 uint64_t edges, moves, candidates, parsimony_start, parsimony; } vdjx_tree_spr_info;          /* 72 bytes */
int vdjx_tree_spr(vdjx_ctx* ctx, const char* contigs, size_t n, int len, const int32_t* clone, const int32_t* anchor, const uint32_t* prio,
                  const int32_t* start_parent /* [nodes] or NULL */, const vdjx_tree_spr_params* params /* NULL: {0, 0} */,
                  int32_t* out_parent, int32_t* out_mutations, int32_t* out_depth, int32_t* out_clone /* each [nodes] */,
                  char* out_anc /* [nodes - n][len]; may be NULL */, vdjx_tree_spr_info* info);

/* ---- weighted (Sankoff) parsimony for the lineage trees ---------------------------------------------------------------------------------
 * vdjx_tree_nj, vdjx_tree_mp and vdjx_tree_spr count every substitution as 1.  Somatic hypermutation prefers transitions, dnapars takes a
 * transversion weight, and phangorn's pratchet / optim.parsimony take a cost matrix and run Sankoff's algorithm.  This call is vdjx_tree_mp
 * with a 4 x 4 cost matrix in place of the unit cost: it scores a rooted tree, optionally runs the same hill climb over nearest-neighbour
 * interchanges under the weighted score, and reconstructs the ancestors and every edge's cost.  It is integer throughout: the device's
 * results are bitwise the model's (tests/tree_sankoff_model.py).  There is no `vdjer` flag for it yet: the call is reached through this
 * header and vdjer_amd.api.
 *   items, start  exactly vdjx_tree_mp's: contigs, n, len, clone[], anchor[], prio, the windows, the local ids (leaves 0 .. m - 1, inferred
 *               nodes m .. 2m - 3), the root member r of smallest (prio, index) with its only child, children kept ascending, the output
 *               slots, start_parent[nodes] or NULL for vdjx_tree_nj's tree, with vdjx_tree_mp's checks.
 *   cost        cost[16], row-major: c[s][t] is the price of a parent in state s over a child in state t (A 0, C 1, G 2, T 3).  The
 *               diagonal must be 0 and every off-diagonal cell 1 .. 65535.  The matrix need not be symmetric and need not satisfy the
 *               triangle inequality: the tree is rooted at r, so the direction is defined.  NULL: every off-diagonal cell 1.  With m <=
 *               4096 a column costs at most 8189 * 65535 < 2^31: per-column quantities fit 32 bits; totals are 64-bit.
 *   up pass     per window column.  A child x's message for a parent state s is H_x(s): c[s][b] for a leaf whose character b is one of
 *               ACGT, 0 for a leaf with any other character (a wildcard, as in vdjx_tree_nj), min_t (c[s][t] + S_x[t]) for an inferred
 *               node, where S_v[s] = H_k0(s) + H_k1(s) over v's two children.  With x the root's child the column costs H_x(b_r) when r's
 *               character is ACGT, otherwise min_s H_x(s).  W(T) is the sum over the columns.  With unit costs W(T) is vdjx_tree_mp's P(T).
 *   down pass   r's state is its base, or for a wildcard the lowest s that minimises H_x(s).  An inferred node x under a parent in state s
 *               takes the lowest t that minimises c[s][t] + S_x[t]; a leaf takes its base, or its parent's state if it is a wildcard.  An
 *               edge's cost is the sum over the columns of c[state(parent)][state(child)], its mutations the number of columns where the
 *               two states differ.  The edge costs sum to W(T).  The ancestors may differ from Fitch's where states tie: Fitch's second
 *               pass picks from the child's set, this rule may keep the parent's state at equal cost.
 *   search      params.search = 1: vdjx_tree_mp's candidates (v, k), swap and m <= 3 rule; a round scores every candidate, the one of
 *               smallest key (W, v, k) is applied if its W is below the current one, otherwise the lineage is finished.  max_rounds as
 *               vdjx_tree_mp's (every move lowers W by at least 1, so the search ends on its own).  With unit costs the moves and the
 *               final parents are vdjx_tree_mp's.  params.search = 0 scores and reconstructs the start tree only.
 *   outputs     [nodes] each.  out_parent, out_mutations, out_depth and out_clone follow vdjx_tree_mp's conventions; out_cost is the cost
 *               of the edge above the node, -1 for a root and for an item in no lineage.  out_anc (may be NULL) is [nodes - n][len], NUL
 *               from w on.
 *   info        (may be NULL; zeroed first) members, clones, largest_clone, internal, batches, edges, moved, moves, rounds as
 *               vdjx_tree_mp's; searched: the lineages of four and more members under search = 1, 0 under search = 0; candidates: the
 *               sum over the lineages and their scoring rounds of 2 (m - 3); cost_start: W of the start trees; cost: the sum of out_cost
 *               over the non-roots (= W of the final trees); mutations: the sum of out_mutations.
 * NOT modelled: TBR under costs (SPR under costs is vdjx_tree_sankoff_spr, below); costs that depend on the 5-mer context or on the column -- Sankoff's
 * recursion needs a cost that depends on the two states alone, so vdjx_sankoff_costs collapses a targeting model to the centre base; a
 * germline node; multifurcations; a `vdjer` flag.
 * VDJX_EINVAL: everything vdjx_tree_mp refuses, with the same messages under this function's name; a cost cell outside the ranges above,
 * named; params.search above 1; a non-zero reserved word -- all before any GPU work.  VDJX_ELIMIT: a lineage of more than
 * VDJX_MP_MAX_MEMBERS members.  n = 0 returns at once with a zeroed info.
 * Batches are vdjx_tree_nj's (whole lineages under VDJX_NJ_CELLS; any value gives the same bytes).  A batch keeps kid, par, W, one int64
 * per candidate and, per (inferred node, column), the node's message H to its parent: four uint32 in one 16-byte vector, the column the
 * fastest index (16 bytes x inferred nodes x columns of workspace; a smaller VDJX_NJ_CELLS cuts it).  Keeping H and not S makes a step of
 * a walk one min-plus product.  The sixteen costs are kernel arguments.  A round is the scorer (a wave per lineage and candidate, 64
 * columns at a time: a lane recomputes v and p and walks to the root against the stored messages of the other children; the cost shows at
 * the root only, as the new root term less the stored one; a wave-wide ballot ends a walk early where no lane's message changed) and
 * pick-and-apply (a workgroup per lineage still searching: block-wide arg-min of (delta in 64 bits, v, k), one thread rewires, all rewrite
 * the stored messages along the path).  The host reads one counter per round from page-locked memory, roots the final kid / par, and the
 * down pass (a wave per lineage and 64 columns, parents before children) writes the states, the ancestors and per edge one integer
 * atomicAdd per wave of its cost (64-bit) and mutations; the search's W must equal the sum of the edge costs (VDJX_ESTATE otherwise).
 * Integer atomics are sums only: two calls give the same bits.  No floating point on the device; scratch comes from the context's
 * workspace.  Stats: "tree_sankoff_us" (host clock over "tree_mp_us"'s span), "tree_sankoff_candidates", "tree_sankoff_steps" (the node
 * updates the scorer made, per candidate and column tile; full rescoring would make candidates x (m - 2) per tile).
 *
 * vdjx_sankoff_costs (plain C, no GPU, no context): a targeting model's weights -> such a matrix, by vdjx_lineage_distance_table's recipe.
 *   weight      uint32 [1024][4] as vdjx_lineage_distance_table takes it (row 256 a + 64 b + 16 c + 4 d + e, column the new base).
 *   cost        Wc[c][e] = the 64-bit sum over the 256 5-mers with centre c of weight[row][e]; w' = max(Wc, 1) for the twelve cells with
 *               e != c; S = their sum; d = -log10((double) w' / (double) S) (libm); mean = the twelve d added left to right in index
 *               order in double, / 12.0; cost[c][e] = floor(1000 * d / mean + 0.5), clamped to 1 .. 65535; the diagonal is 0.  A uniform
 *               model gives 1000 everywhere.
 *   info        (may be NULL) mean, and the smallest and largest off-diagonal cell.
 * VDJX_EINVAL: a NULL weight or cost. */
typedef struct { uint32_t max_rounds, search, reserved[2]; } vdjx_tree_sankoff_params;      /* 16 bytes; reserved must be 0, search 0 or 1 */
typedef struct { uint32_t members, clones, largest_clone, internal, batches, searched, moved, rounds;
                 uint64_t edges, moves, candidates, cost_start, cost, mutations; } vdjx_tree_sankoff_info;     /* 80 bytes */
typedef struct { double mean; uint32_t min_cost, max_cost; } vdjx_sankoff_costs_info;       /* 16 bytes */
int vdjx_tree_sankoff(vdjx_ctx* ctx, const char* contigs, size_t n, int len, const int32_t* clone, const int32_t* anchor, const uint32_t* prio,
                      const uint32_t* cost /* [16] or NULL */, const int32_t* start_parent /* [nodes] or NULL */,
                      const vdjx_tree_sankoff_params* params /* NULL: {0, 1, {0, 0}} */, int32_t* out_parent, int64_t* out_cost,
                      int32_t* out_mutations, int32_t* out_depth, int32_t* out_clone /* each [nodes] */,
                      char* out_anc /* [nodes - n][len]; may be NULL */, vdjx_tree_sankoff_info* info);
int vdjx_sankoff_costs(const uint32_t* weight /* [1024][4] */, uint32_t* cost /* [16] */, vdjx_sankoff_costs_info* info);

/* ---- subtree pruning and regrafting under Sankoff costs -----------------------------------------------------------------------------------
 * vdjx_tree_spr searches by subtree pruning and regrafting but counts every substitution as 1; vdjx_tree_sankoff scores under a cost
 * matrix but moves by nearest-neighbour interchanges only.  dnapars (with a transversion weight) and phangorn's pratchet /
 * optim.parsimony (with a cost matrix) rearrange by SPR under that weight.  This call is vdjx_tree_spr's search under
 * vdjx_tree_sankoff's score.  It is integer throughout: the device's results are bitwise the model's
 * (tests/tree_sankoff_spr_model.py).  There is no `vdjer` flag for it yet: the call is reached through this header and vdjer_amd.api.
 *   items, start  exactly vdjx_tree_mp's: contigs, n, len, clone[], anchor[], prio, the windows, the local ids (leaves 0 .. m - 1, inferred
 *               nodes m .. 2m - 3), the root member r of smallest (prio, index) with its only child, children kept ascending, the output
 *               slots, start_parent[nodes] or NULL for vdjx_tree_nj's tree, with vdjx_tree_mp's checks; batches under VDJX_NJ_CELLS.
 *   cost, up pass, down pass, outputs   exactly vdjx_tree_sankoff's: cost[16] (c[s][t]: a parent in state s over a child in state t; the
 *               diagonal 0, the rest 1 .. 65535; NULL: all 1) and its refusals, the messages H_x(s), S_v, the column cost, W(T), the down
 *               pass, out_cost, out_mutations, out_anc.
 *   candidates, apply   exactly vdjx_tree_spr's: a lineage of m >= 4 members is searched; (c, y) with c any node other than r and r's
 *               child, T' the tree without c's subtree and with p = parent(c) dissolved (s, p's other child, under g = parent(p)), y any
 *               node of T' other than r and s; the apply rule; params.max_rounds caps a lineage's scoring rounds (0: until finished).
 *   round       one round of one lineage scores every candidate; the one of smallest key (W, c, y) is applied if its W is below the
 *               current W, otherwise the lineage is finished.  Every move lowers W by at least 1, so the search ends on its own.  Where
 *               costs tie the key is the definition.  With unit costs -- and with any matrix whose twelve costs are equal -- the moves
 *               and the final parents are vdjx_tree_spr's.
 *   info        (may be NULL; zeroed first) vdjx_tree_sankoff_info; candidates as vdjx_tree_spr counts them (per round, tree-dependent);
 *               searched: the lineages of four and more members.
 * With m <= VDJX_SPR_MAX_MEMBERS a column's quantities (messages, E', a candidate's cost, the sums inside a min-plus step) are below
 * 2046 x 65535 < 2^31 and are kept in 32 bits; totals, deltas and the keys' deltas are 64-bit.
 * The scorer's identity.  Fitch's root-independence, which vdjx_tree_spr uses, does not hold for an asymmetric matrix.  With H' the
 * messages of T' -- the stored H except on the path from g to r, where they are recomputed upwards from S'_g = H_s + H_other -- and
 * E'_y(u) the cheapest cost of everything in T' outside y's subtree plus the edge into a node in state u placed directly above y:
 *     E'_top(u) = c[b_r][u] for top, r's child in T' (0 for all u where r's character is a wildcard),
 *     E'_y(u) = min_v (E'_x(v) + H'_z(v) + c[v][u]) for the children y, z of an inferred node x,
 *     W(T after (c, y)) = sum over the columns of min_u (E'_y(u) + H_c(u) + H'_y(u)).
 * A round is the scorer (a wave per lineage and pruned node, 64 columns at a time: the path walk, then one pre-order walk of T'; a 16-byte
 * vector per (node, lane) that holds first H' and then E', in LDS up to 32 members, in the workspace beyond; O(m^2 w) per lineage and
 * round) and pick-and-apply (a workgroup per lineage still searching: arg-min of (delta in 64 bits, c, y), one thread rewires, all rewrite
 * the stored messages along the two changed paths).  The host reads one counter per round from page-locked memory, roots the final kid /
 * par, and vdjx_tree_sankoff's down pass runs unchanged; the search's W must equal the sum of the edge costs (VDJX_ESTATE otherwise).
 * Integer atomics are sums only: two calls give the same bits.  No floating point; scratch comes from the context's workspace.
 * NOT modelled: TBR; random restarts and the parsimony ratchet; multifurcations; a germline node; costs that depend on the 5-mer context
 * or on the column; a `vdjer` flag.
 * VDJX_EINVAL: everything vdjx_tree_sankoff refuses (but params.search, which this call has not), with the same messages under this
 * function's name; a non-zero reserved word -- all before any GPU work.  VDJX_ELIMIT: a lineage of more than VDJX_SPR_MAX_MEMBERS
 * members, refused as vdjx_tree_spr refuses it.  n = 0 returns at once with a zeroed info.
 * Stats: "tree_sankoff_spr_us" (host clock over "tree_mp_us"'s span), "tree_sankoff_spr_candidates". */
typedef struct { uint32_t max_rounds, reserved[3]; } vdjx_tree_sankoff_spr_params;   /* 16 bytes; reserved must be 0 */
int vdjx_tree_sankoff_spr(vdjx_ctx* ctx, const char* contigs, size_t n, int len, const int32_t* clone, const int32_t* anchor,
                          const uint32_t* prio, const uint32_t* cost /* [16] or NULL */, const int32_t* start_parent /* [nodes] or NULL */,
                          const vdjx_tree_sankoff_spr_params* params /* NULL: all 0 */, int32_t* out_parent, int64_t* out_cost,
                          int32_t* out_mutations, int32_t* out_depth, int32_t* out_clone /* each [nodes] */,
                          char* out_anc /* [nodes - n][len]; may be NULL */, vdjx_tree_sankoff_info* info);

/* ---- split support for the trees with inferred ancestors: the delete-half jackknife around neighbour joining ---------------------------
 * vdjx_tree_nj and vdjx_tree_mp give a fully resolved tree, and nothing in it says which internal edges the data decides.  This call gives
 * what dowser's getBootstraps and ape's boot.phylo print on the internal nodes of a Newick tree: for every inferred node, the number of
 * replicates whose tree has the same split.  vdjx_tree_support's figure counts edges {i, parent[i]} between two items, which a tree with
 * inferred nodes does not have.  Integer throughout: the device's results are bitwise the model's (tests/tree_split_model.py).  There is
 * no `vdjer` flag for it yet: the call is reached through this header and vdjer_amd.api / vdjer_amd.annot.
 *   items       contigs, n, len, clone[], anchor[], prio exactly as vdjx_tree_nj takes them: the same windows (a, b), w = a + b, the same
 *               local leaf ids 0 .. m - 1 in ascending caller index, the same root (the member of smallest (prio, index)).
 *   parent      [nodes], nodes = vdjx_tree_nj_nodes(clone, n), in vdjx_tree_nj's slots: the scored tree.  Any rooted binary tree that
 *               vdjx_tree_mp would accept as start_parent -- vdjx_tree_nj's out_parent, vdjx_tree_mp's, or a handmade one -- checked as
 *               there and refused with the same kind of message.
 *   splits      clade(v) of an inferred node v: the members below it.  The tree is rooted at a leaf, so clade(v) is the side of the edge
 *               (v, parent(v)) without the root member, and two trees over the same members share that bipartition iff they have a node
 *               of the same clade.  The root's only child (everyone but the root) and the leaves are trivial and not scored: a lineage of m
 *               members has max(0, m - 3) scored nodes, the internal edges of an unrooted binary tree.
 *   replicate   r = 1 .. replicates keeps window position q when bit q & 31 of mix64(seed ^ ((uint64_t) r << 32 | q >> 5)) is set:
 *               vdjx_tree_support's rule bit for bit, the same for every lineage (the same seed deletes the same columns there and
 *               here).  d_r(i, j) is the distance over the kept positions alone; the replicate's tree is vdjx_tree_nj's joining on
 *               D = d_r << 16 -- the same key (Q, i, j), the same floors, the same node ids in creation order -- rooted at the same member.
 *               A replicate that keeps no position of a lineage's window has all distances 0: the key still defines its tree.  Branch
 *               lengths and Fitch's passes are not computed.
 *   output      out_support[v], for a scored node v: the number of replicates whose tree has an inferred node with exactly clade(v)
 *               (equality of sets, not of a hash).  -1 in every other slot: items, the root's child, the nodes of lineages of three and
 *               fewer, items with clone = -1.  out_rep_parent (may be NULL) is [replicates][nodes]: every replicate's rooted tree in
 *               vdjx_tree_nj's slots -- what vdjx_tree_nj's joining gives on the kept columns, the lineages of three and fewer included --
 *               so that a support can be traced to the replicate that made it.
 *   info        (may be NULL; zeroed first, every field filled on success) members, clones, largest_clone as vdjx_tree_nj's; replicates;
 *               batches; units: the (replicate, lineage of four and more) pairs; scored: the scored nodes; matched: the sum of the
 *               supports; full: the scored nodes with support = replicates; joins, cells: vdjx_tree_nj's, summed over the units.
 * NOT modelled: a parsimony search per replicate (for vdjx_tree_mp's and vdjx_tree_spr's trees the replicates are still neighbour-joining
 * trees); the bootstrap
 * with replacement; a consensus tree of the replicates.
 * VDJX_EINVAL: everything vdjx_tree_nj refuses; replicates outside 1 .. 1024; reserved != 0; a parent that vdjx_tree_mp would refuse as a
 * start; NULL parent, params or out_support.  VDJX_ELIMIT: a lineage of more than VDJX_NJ_MAX_MEMBERS members.  All before any GPU work.
 * n = 0 returns at once with a zeroed info.
 * The host lays the lineages out, checks the scored tree and makes its canonical clades (bitsets of ceil(m / 64) 64-bit words over the
 * local leaf ids) with their signatures, sorted, once per lineage.  The units run replicate-major in batches of whole units of at most
 * VDJX_NJ_CELLS matrix cells (vdjx_tree_nj's knob, read per call; any value gives the same bytes).  A batch: the pack through the
 * replicates' kept positions; vdjx_tree_nj's matrix and join kernels unchanged (a unit is a lineage to them); the clades of the join order
 * (a wave per unit, a lane per word: a join's clade is the union of its two children's, one pass in creation order; complemented within m
 * bits where it holds the root; in LDS up to 64 members); the look-up (a lane per clade: up to 64 members the one word is searched for,
 * beyond that the wrap-around sum of mix64(leaf + 1), then the run of equal signatures; a hit counts after all words compare equal: one
 * integer atomicAdd).  Nothing is read back per batch unless out_rep_parent is given (then the edges, rooted on the host); the supports come
 * back once.  Sums only: two calls give the same bits.  No floating point; scratch comes from the context's workspace.  Stats:
 * "tree_split_us" (host clock), "tree_split_units", "tree_split_batches".
 *
 * vdjx_tree_split_compare is the match step on the host, exactly (plain C, no GPU): out_shared[v] is 1 or 0 for a scored node v of tree a
 * -- whether tree b has its clade -- and -1 elsewhere; *shared and *scored (may be NULL) count them.  The Robinson-Foulds distance of two
 * trees, such as vdjx_tree_nj's and vdjx_tree_mp's, is 2 (scored - shared).  A lineage's root in either tree is its member without a parent;
 * the clades of both are taken against tree a's root.  Refused (VDJX_EINVAL) with vdjx_tree_mp's messages for a bad start_parent, and when
 * nodes is not vdjx_tree_nj_nodes(clone, n). */
typedef struct { uint32_t replicates; uint32_t reserved; uint64_t seed; } vdjx_tree_split_params;               /* 16 bytes; reserved must be 0 */
typedef struct { uint32_t members, clones, largest_clone, replicates, batches, units;
                 uint64_t scored, matched, full, joins, cells; } vdjx_tree_split_info;                          /* 64 bytes */
int vdjx_tree_split_support(vdjx_ctx* ctx, const char* contigs, size_t n, int len, const int32_t* clone, const int32_t* anchor, const uint32_t* prio,
                            const int32_t* parent /* [nodes] */, const vdjx_tree_split_params* params, int32_t* out_support /* [nodes] */,
                            int32_t* out_rep_parent /* [replicates][nodes] or NULL */, vdjx_tree_split_info* info);
int vdjx_tree_split_compare(const int32_t* clone, size_t n, const int32_t* parent_a, const int32_t* parent_b, uint64_t nodes,
                            int32_t* out_shared /* [nodes] */, uint64_t* shared, uint64_t* scored);

/* ---- germline rows and R/S mutation counts: the contig and its V(D)J germline side by side, classified codon by codon ----------------
 * gives `vdjer --mutations` what Change-O's CreateGermlines and shazam's observedMutations make of V'DJer's output in a second tool: the
 * sequence_alignment / germline_alignment / germline_alignment_d_mask rows and the replacement / silent mutation counts of the V segment.
 * All arithmetic is integer: the device's results are bitwise the model's (tests/mutation_model.py).
 *   inputs      contigs, n, len as vdjx_annotate takes them; v[n], j[n] and d[n] (d may be NULL) are hits as vdjx_annotate / vdjx_dcall
 *               return them, but any CONSISTENT hit is accepted (the VDJX_EINVAL list below is what consistent means); limit[n] (NULL:
 *               len for every contig) bounds the contig positions whose V mutations are counted.  A hit is USABLE when gene >= 0, score >
 *               0 and n_runs <= VDJX_ANNOT_RUNS; a hit with gene >= 0, score > 0 and more than 64 runs has no runs to read: it is treated
 *               as absent, sets flag 16 and counts in info->truncated (per hit).  gene indexes the records as they were given to
 *               vdjx_germline_load (v, j) or vdjx_dsegment_load (d).  A germline base whose stored code is not ACGT prints as N.
 *   columns     of contig i, V usable; the alignment starts at contig position v.seq_start:
 *               1. V columns, from V's runs 5' to 3': an M run of k gives k columns (contig base, germline base), an I run (contig
 *                  base, '-'), a D run ('-', germline base).
 *               2. J, when usable: j.seq_start > v.seq_end keeps all its columns.  Otherwise J is clipped (flag 8, info->clipped): its
 *                  columns are dropped from its 5' end up to, not including, the first column that carries a contig base at a position >
 *                  v.seq_end (D columns directly before it go too); when there is no such column J is not used (flag 8 stays set).
 *               3. gap columns, when J is used: g0 = v.seq_end, g1 = the contig position of J's first kept contig base - 1; the gap is the
 *                  contig positions g0 + 1 .. g1 (empty whenever J was clipped).  With d given, d[i] usable, d.seq_start > g0 and d.seq_end
 *                  <= g1: np1 = d.seq_start - g0 - 1 columns (contig base, 'N'), the D hit's columns by its runs as for V, np2 = g1 -
 *                  d.seq_end columns (contig base, 'N').  Otherwise every gap column is (contig base, 'N').
 *               4. J's kept columns, by its runs.
 *               5. J not used: the alignment ends after the V columns and D is not used.
 *   rows        sequence_alignment: the columns' first members; germline_alignment: the second; germline_alignment_d_mask: the germline
 *               row with N in EVERY column between the last V and the first J column, the D hit's own deletion columns included (so the
 *               three rows are equally long): CreateGermlines' default dmask, the row shazam reads.  No usable V: cols = 0, empty rows,
 *               every count 0.
 *   V counts    a V record is taken to begin with the first base of a codon (IMGT V-REGION records do): germline codon c is the record's
 *               bases 3c .. 3c+2 (0-based).  A codon is CLASSIFIABLE when it lies inside germ_start .. germ_end, each of its three bases
 *               is in an M column, those three columns are adjacent (no I between them), the three contig positions are all < limit[i]
 *               (0-based) and all six characters are upper-case ACGT.  v_codons counts them.  Each position of a classifiable codon at
 *               which contig and germline differ is classified on its own, in the germline's context (shazam's rule for codons with
 *               several mutations): take the germline codon with that one base replaced by the contig's; the germline codon or the changed
 *               one is a stop: v_stop; else both translate alike: v_s; else v_r.  The genetic code is the standard one.  v_na counts
 *               every other V M column at a contig position < limit[i] whose two characters differ or are not both ACGT.  So v_r + v_s +
 *               v_stop + v_na = the V mismatch columns below the limit by vdjx_annotate's meaning of a mismatch (v.mismatches when limit
 *               >= v.seq_end).  j_mis: the kept J M columns that mismatch (J has no frame of its own here: no R/S).
 *   row         cols and the counts; flags: 1 V used, 2 J used, 4 D used, 8 J clipped, 16 a hit of this contig had more than 64 runs.
 *   info        (may be NULL; zeroed first, summed from the rows on the host) contigs = n; aligned: rows with flag 1; cols .. v_codons:
 *               the sums; truncated: hits over 64 runs; clipped: rows with flag 8.
 *   layout      vdjx_mutations_layout (host only; no context) computes every contig's columns from the hits alone: out_off[i] is where
 *               contig i's rows start in each of the three row buffers, out_off[n] the size of each.  Deletions make cols exceed len.
 *   output      contig i's rows go to out_seq / out_germ / out_mask + out_off[i], cols bytes, no terminator; each of the three may be
 *               NULL.  out_rows is required.
 * NOT modelled: IMGT gaps and numbering (the CDR / FWR split of the counts by the caller's intervals, the expected counts under a
 * targeting model and the selection strength are vdjx_selection's, below); V records that begin inside a codon (IMGT's 5'-partial
 * sequences: their codons are shifted); R/S for the J segment; a clonal consensus germline (CreateGermlines --cloned; the clone's own
 * consensus is vdjx_consensus, below); a germline node as
 * the root of `--trees`.
 * VDJX_EINVAL (the message names the contig): a usable hit whose gene is out of range or names a record of the wrong class (v: 'V', j:
 * 'J'); germ_end past the record's end; seq_start or germ_start < 1, seq_end > len; a run with an op outside 0..2 or a length of 0; M + I
 * run lengths that do not sum to seq_end - seq_start + 1, M + D run lengths that do not sum to germ_end - germ_start + 1; a limit outside
 * 0 .. len; contigs of unequal length (a NUL inside the n*len characters), len >= 4096, n >= 2^20; NULL out_rows.  VDJX_ESTATE: no
 * germline set is loaded, or d is given and no D set is loaded.  n = 0 returns at once with a zeroed info.  The host checks the hits,
 * computes the layout and uploads per contig 64 bytes of positions and record offsets and its usable runs (4 bytes each), not 340 bytes
 * per hit.  A call is ONE kernel dispatch (scope "k_mutations") whatever n is.  Scratch comes from the context's workspace; no floating
 * point, no atomics: two calls give the same bits.  Stats: "mutations_cols" (out_off[n]), "mutations_us" (host clock). */
typedef struct { int32_t cols, v_r, v_s, v_stop, v_na, v_codons, j_mis, flags; } vdjx_mut_row;      /* 32 bytes */
typedef struct { uint64_t contigs, aligned, cols, v_r, v_s, v_stop, v_na, v_codons; uint32_t truncated, clipped; } vdjx_mut_info;   /* 72 bytes */
int vdjx_mutations_layout(const vdjx_annot_hit* v, const vdjx_annot_hit* d, const vdjx_annot_hit* j, size_t n, uint64_t* out_off /* n + 1 */);
int vdjx_mutations(vdjx_ctx* ctx, const char* contigs, size_t n, int len, const vdjx_annot_hit* v, const vdjx_annot_hit* d,
                   const vdjx_annot_hit* j, const int32_t* limit, char* out_seq, char* out_germ, char* out_mask,
                   vdjx_mut_row* out_rows, vdjx_mut_info* info);

/* ---- selection strength: observed against expected R / S of the V segment, and the posterior of sigma (BASELINe) ----------------------
 * gives `vdjer --selection` what shazam's expectedMutations / calcBaseline / groupBaseline / summarizeBaseline make of the mutation counts
 * in a second tool: whether the replacement share departs from what the germline's codons and the mutation process alone would give.  The
 * counts and weights are integer: the device's are bitwise the model's (tests/selection_model.py).  The posterior is float64.
 *   inputs      contigs, n, len, v[n] and limit[n] as vdjx_mutations takes them (no J, no D).  cdr: the region map (below) or NULL;
 *               weight: the targeting model, uint32 [1024][4], or NULL (uniform); group[n]: the group 0 .. G - 1 of every contig, negative:
 *               in no group (may be NULL when G = 0).
 *   observed    the classifiable codons of the V hit exactly as vdjx_mutations defines them, limit included; each differing base is
 *               classified as there (R, S or stop) and counted in the REGION of the germline position that carries the base; stops are
 *               counted in neither obs_r nor obs_s.  A codon is counted (codons) in the region of its first base.  Summed over the regions
 *               obs_r, obs_s and codons are vdjx_mutations' v_r, v_s and v_codons.
 *   expected    (integer, exact) for every base position p of a classifiable codon whose germline codon is not a stop, and each of the
 *               three other bases b: the germline codon with b at p is a stop: nothing; it translates like the germline codon: w goes to
 *               exp_s; otherwise w goes to exp_r -- of the region of p.  w = weight[idx5(p)][b], idx5 = 256 g[p-2] + 64 g[p-1] + 16 g[p] +
 *               4 g[p+1] + g[p+2] (A 0, C 1, G 2, T 3) over the RECORD's bases, not the hit's; one of the five outside the record or not
 *               ACGT: the position adds nothing.  weight == NULL: w = 1 at every position, whatever its neighbours.  Weights are uint32,
 *               sums uint64.  (The entry weight[..][g[p]] of the centre base itself is never read.)
 *   region map  cdr: four int32 per record, indexed by the record index given to vdjx_germline_load (n_records rows): cdr1_start,
 *               cdr1_end, cdr2_start, cdr2_end; 1-based, inclusive, ungapped positions of the record; 0, 0: no such interval.  A position
 *               inside either interval is CDR (region 1), every other is FWR (region 0).  A record whose first entry is -1 has no regions:
 *               its contigs take no part (flag 32, all counts 0, info->no_regions).  Rows of records that are not V records are not read.
 *               cdr == NULL: one region, the whole V (K = 1); otherwise K = 2.
 *   counts      out_counts[i]: obs_r, obs_s, codons, exp_r, exp_s per region (index 1 is 0 when K = 1); flags: 1 V used, 16 the hit has
 *               more than 64 runs (treated as absent, as in vdjx_mutations), 32 the V record has no regions.
 *   statistic   (BASELINe's focused test; its local test when K = 1) contig i in region k: x = obs_r[k], n = obs_r[k] + the sum over the
 *               regions of obs_s, odds exp_r[k] : the sum over the regions of exp_s.  A contig with n = 0, exp_r[k] = 0 or that sum 0 adds
 *               nothing to region k and is not counted in `sequences`.
 *   posterior   on the fixed grid sigma_t = (t - 2000) / 100, t = 0 .. 4000 (VDJX_SEL_GRID points, -20 .. 20).  For a row (a set of
 *               contigs) and a region, with softplus(z) = max(z, 0) + log1p(exp(-|z|)):
 *                   l(sigma) = sigma - 2 softplus(sigma) + sum over the members of [ x_i z_i - n_i softplus(z_i) ],
 *                   z_i = sigma + ln(exp_r_i) - ln(exp_s_i)
 *               The first term is the prior, a standard logistic on sigma centred on no selection (a uniform prior on the replacement share
 *               when the expected share is 1/2); the sum is the binomial log-likelihood of a shared sigma with every member's own expected
 *               odds.  f_t = exp(l_t - max l), S = sum f_t; pdf_t = f_t / (0.01 S); sigma = sum sigma_t f_t / S; cdf_t = sum over u <= t
 *               of f_u / S; lower (upper): sigma_t of the first t with cdf_t >= 0.025 (0.975); p_positive = (sum over t > 2000 of f_t + f_2000
 *               / 2) / S.
 *   rows        one per contig (a set of one), one per group 0 .. G - 1, one last for all contigs: n + G + 1 rows of K regions;
 *               out_stat[row * K + region].  sequences: the contributing members; x, n, exp_r, exp_s: their sums.  A row without one is
 *               the prior alone: sigma 0, p_positive 1/2.  out_pdf (may be NULL): the densities of the G + 1 group and sample rows,
 *               [(G + 1)][K][VDJX_SEL_GRID].
 *   info        (may be NULL; zeroed first) contigs = n; used: rows with flag 1; no_regions: flag 32; truncated: flag 16; groups = G;
 *               regions = K; chunks: the partial sums of large rows (below), over both regions; large_rows: the rows that had them.
 * A group row here is a SHARED sigma; shazam's group density -- the convolution of the members' densities -- and the comparison of two groups'
 * densities are vdjx_selection_convolve and vdjx_selection_compare, below.
 * NOT modelled: shazam's fitted priors (BAYESIAN_FITTED); IMGT numbering (the regions are the caller's intervals); N-averaged 5-mers; one
 * representative per clone for the sample row (run it on vdjx_consensus_hits' pseudo-contigs for that); the J segment.
 * VDJX_EINVAL (the message names the contig or the record): vdjx_mutations' list for the contigs, the V hits and the limit; n_records is not
 * the number of records given to vdjx_germline_load; an interval of a V record with start > end, start < 1 or end past the record; group[i]
 * >= G; G >= 2^20; out_pdf with G + 1 > 65,536; NULL out_counts or out_stat.  VDJX_ESTATE: no germline set is loaded.  n = 0 returns at
 * once with a zeroed info.  Three kernels: k_sel_counts (one dispatch, a wave per contig; integer only, no atomics), then on the host the
 * members' x, n and log-odds and ONE sort of the members by group; k_sel_loglik only for rows of more than `chunk` members (VDJX_SEL_CHUNK,
 * 1 .. 65,536, default 1024, read per call): a row's members are cut into chunks in order and every chunk's sum over its members, in
 * contig order, is stored per grid point -- at most 2n / chunk + G + 1 chunks per region; k_sel_finish, a workgroup per (row, region), adds a
 * row's chunks in order (or its members directly) to the prior and reduces.  No float atomics, every sum in a fixed order: two calls with
 * the same VDJX_SEL_CHUNK give the same bits.  Scratch comes from the context's workspace.  Stats: "selection_us" (host clock),
 * "selection_chunks". */
#define VDJX_SEL_GRID 4001
typedef struct { int32_t obs_r[2], obs_s[2], codons[2]; uint32_t flags, pad; uint64_t exp_r[2], exp_s[2]; } vdjx_sel_counts;   /* 64 bytes */
typedef struct { uint32_t sequences, pad; uint64_t x, n, exp_r, exp_s; double sigma, lower, upper, p_positive; } vdjx_sel_stat;   /* 72 bytes */
typedef struct { uint64_t contigs, used, no_regions, truncated; uint32_t groups, regions, chunks, large_rows; } vdjx_sel_info;    /* 48 bytes */
int vdjx_selection(vdjx_ctx* ctx, const char* contigs, size_t n, int len, const vdjx_annot_hit* v, const int32_t* limit, const int32_t* cdr,
                   size_t n_records, const uint32_t* weight /* 1024 * 4, or NULL */, const int32_t* group, uint32_t G,
                   vdjx_sel_counts* out_counts /* n */, vdjx_sel_stat* out_stat /* (n + G + 1) * K, row-major */,
                   double* out_pdf /* NULL, or (G + 1) * K * 4001: the group rows, then the sample row */, vdjx_sel_info* info);

/* ---- BASELINe's group posteriors: the members' own posteriors, convolved; and the comparison of two densities ------------------------------
 * gives `vdjer --selection-combine mean` and `--selection-test` what shazam's groupBaseline / summarizeBaseline / testBaseline make of the
 * members' densities: the density of a row is the distribution of the weighted MEAN of its members' independent sigmas, in which every
 * member counts once, not the posterior of one sigma shared by all of them.  The model in Python: tests/selection_conv_model.py.
 *   inputs      counts[n]: the count rows vdjx_selection returned (or handmade ones; only obs_r, obs_s, exp_r and exp_s are read); K: the
 *               regions, 1 or 2; group[n] and G as vdjx_selection takes them.  Rows: the G groups, then all contigs; out_stat[row * K +
 *               region], out_pdf (may be NULL) [(G + 1)][K][VDJX_SEL_GRID].
 *   leaves      the contributing members of a row in a region are those vdjx_selection counts in `sequences` (n > 0, exp_r[k] > 0, the sum
 *               of exp_s > 0), in contig order.  Member i's leaf is its own posterior as a MASS vector m_i[t] = f_t / S, f and S as
 *               vdjx_selection defines them for a row holding that member alone (the prior times its likelihood); weight 1.
 *   tree        depends only on the number m of leaves: a row of one is its leaf; a row of m > 1 combines the result of its first
 *               h = 2^(ceil(log2 m) - 1) leaves (weight h) with the result of the other m - h.  (Rounds of adjacent pairs with an odd last
 *               entry passed through build this tree, and so does a binary counter over blocks of leaves.)
 *   combine     (A, a) (+) (B, b) -> (C, a + b): the distribution of (a sigma_A + b sigma_B) / (a + b), put back on the grid by mass-
 *               conserving linear binning.  With u, v = -2000 .. 2000 (grid index - 2000), den = a + b, num = a u + b v, q = floor(num / den),
 *               rem = num - q den (integers): the mass A[u] B[v] goes to C[q] with the share (den - rem) / den and to C[q + 1] with rem / den;
 *               with rem = 0 cell q + 1 gets nothing and is neither read nor written (u = v = 2000: q + 1 is past the grid).  Equivalently
 *               C[c] = sum over |a u + b v - c den| < den of A[u] B[v] (den - |a u + b v - c den|) / den.  All terms are non-negative; in
 *               exact arithmetic the sum of C is 1 and its mean the weighted mean of the means.
 *   root        S' = sum C; pdf_t = C[t] / (0.01 S'); sigma, lower, upper and p_positive from C / S' by vdjx_selection's rules (the quantiles
 *               are grid points; half of grid point 0 counts as positive).  sequences, x, n, exp_r, exp_s: the members' sums, as there.  A
 *               row without a contributing member is the prior: sigma 0, p_positive 1/2.
 *   order       no floating-point atomics; one thread owns an output cell and sums its terms in a register.  a = b: B'[s] = (B[s - 1] / 2 +
 *               B[s]) + B[s + 1] / 2 first, then C[c] = sum over u ASCENDING of A[u] B'[2c - u], one fused multiply-add per term.  a > b (the
 *               left side of a tree's combination is never the lighter one): v ascending, inside it u ascending, each term (A[u] B[v]) *
 *               ((den - |a u + b v - c den|) * (1 / den)).  Two calls give the same bits, with any VDJX_CONV_CELLS.
 *   info        (may be NULL; zeroed first) members: the contributing members summed over rows and regions; leaves: the leaf densities
 *               evaluated (members, plus one prior per row and region without a member); combines; groups = G; regions = K; rows = (G + 1)
 *               K; levels: the deepest tree, ceil(log2 m); batches.
 * VDJX_EINVAL: K outside 1 .. 2; group[i] >= G; G >= 2^20; n >= 2^20; out_pdf with G + 1 > 65,536; G > 0 without a group array; NULL counts
 * or out_stat.  n = 0 returns at once with a zeroed info.  Needs no germline set.  Three kernels: k_conv_leaf (a workgroup per leaf),
 * k_conv_combine (one launch per level of the rows in flight; a workgroup per combination and tile of 256 output cells, both densities in
 * LDS) and k_conv_finish (a workgroup per row); the host lays out every launch of the call first, nothing is read back in between.  A
 * density is 32 KB: VDJX_CONV_CELLS (4 .. 2^20, default 32,768 = 1 GB, read per call) is the number held at once.  Whole rows go in batches
 * (a row of m leaves holds m + m / 2 densities at its first level); a row that does not fit goes alone, in blocks of a power of two of leaves
 * whose roots meet on a stack the way a binary counter's digits do -- the same tree, so the same bits -- and holds ceil(log2 m) + 3 densities
 * even where the knob asks for fewer.  Scratch comes from the context's workspace.  Stats: "selconv_us" (host clock), "selconv_combines",
 * "selconv_batches".
 *
 * vdjx_selection_compare (plain host code, needs no device and no context; shazam's testBaseline): pdf holds `rows` densities of
 * VDJX_SEL_GRID values each (any positive scale: each is divided by its own sum); pair[P][2] names the rows a and b of every comparison.
 *   p_greater = sum over t ascending of a[t] (sum over s < t of b[s] + b[t] / 2): P(sigma_a > sigma_b) plus half of P(equal); float64, at most 1.
 *   pvalue = min(1, 2 min(p_greater, 1 - p_greater)).   fdr: Benjamini-Hochberg over the P' comparisons that are not skipped, sorted
 *   ascending by pvalue with ties in row order: fdr_(i) = min(1, min over j >= i of pvalue_(j) P' / j).   skip (may be NULL): 1 leaves the
 *   comparison's three values 0 and out of the fdr.   VDJX_EINVAL: a row index >= rows; NULL pdf, pair or out (with P > 0).
 * NOT modelled: shazam's fitted priors; the FFT resampling of its weighted_conv (the binning here is linear); comparisons between lineages
 * and groupings other than lineages on vdjer's command line (this call takes any grouping, that one any pair of rows). */
typedef struct { uint64_t members, leaves, combines; uint32_t groups, regions, rows, levels, batches, pad; } vdjx_selconv_info;   /* 48 bytes */
typedef struct { double p_greater, pvalue, fdr; } vdjx_sel_test;                                                                /* 24 bytes */
int vdjx_selection_convolve(vdjx_ctx* ctx, const vdjx_sel_counts* counts, size_t n, uint32_t K /* 1 or 2 */, const int32_t* group, uint32_t G,
                            vdjx_sel_stat* out_stat /* (G + 1) * K: the groups, then all contigs */,
                            double* out_pdf /* NULL, or (G + 1) * K * 4001 */, vdjx_selconv_info* info);
int vdjx_selection_compare(const double* pdf, size_t rows, const uint32_t* pair /* P x 2: row a, row b */, size_t P,
                           const uint8_t* skip /* NULL, or P: 1 = leave the row empty and out of the fdr */, vdjx_sel_test* out);

/* ---- the sample's own 5-mer targeting model: which 5-mers mutate, and to which base (S5F) ---------------------------------------------
 * gives `vdjer --targeting-model` what shazam's createTargetingModel (createSubstitutionMatrix, createMutabilityMatrix,
 * createTargetingMatrix) makes of the sample in a second tool: the weights vdjx_selection takes, learnt from the V segments at hand.
 * Everything on the device is integer: its counts are bitwise the model's (tests/targeting_model.py).
 *   inputs      contigs, n, len, v[n], limit[n] and group[n] as vdjx_selection takes them; no region map, no weights, no G: any group[i]
 *               >= 0 is a group, a negative one (or group == NULL) leaves the contig on its own.  A hit with more than 64 runs is treated
 *               as absent (info->truncated).
 *   units       a unit is a pair (group, V record); a contig in no group is a unit of its own.  A unit owns 4 bits per 0-based record
 *               position p.
 *   marking     for every contig, every codon vdjx_mutations classifies (limit included) whose germline codon is not a stop, and every base
 *               p of it that has a 5-mer -- vdjx_selection's rule: p >= 2, p + 2 < the record's length, the four neighbours in the RECORD
 *               are ACGT -- with gb the germline's and cb the contig's base code (A 0, C 1, G 2, T 3): bit gb of p is set ("seen"); if cb !=
 *               gb and the germline codon with this ONE base replaced is not a stop, bit cb of p is set.  Each base is judged on its own.
 *   counting    out[kind][class][m][x], kind 0 observed, 1 opportunity; class 0 silent, 1 replacement; m = idx5(p) as vdjx_selection forms
 *               it; x the new base.  For every seen p of every unit and every x != gb whose substituted codon is no stop: the opportunity of
 *               x's class + 1, and if bit x of p is set the observed count + 1.  The entries x == gb stay 0.
 *               The result is a function of the SET of bits: it does not depend on the order of the contigs, on which member set a bit or
 *               on the batches.  A mutation the members of a lineage share over one record is one event; the same change over two records
 *               of one lineage is two.
 *   info        (may be NULL; zeroed first) contigs = n; used: the contigs with a usable V hit; truncated; units; positions: the seen
 *               bits; obs_s, obs_r, opp_s, opp_r: the four tables' sums; batches.
 * VDJX_EINVAL (the message names the contig): vdjx_selection's list for the contigs, the V hits and the limit; NULL out.  VDJX_ESTATE: no
 * germline set is loaded.  n = 0 returns at once with a zeroed info and zeroed counts.  The host orders the contigs by unit and cuts the units
 * into batches of VDJX_TGT_UNITS (1 .. 2^20 - 1, default 2^18, read per call; 1 KB of bitmap each, from the context's workspace); any value
 * gives the same counts.  Per batch one memset and two kernels: k_tgt_mark (a wave per contig, 32-bit atomicOr into the unit's words) and
 * k_tgt_count (a wave per unit, a 48 KB histogram in LDS per workgroup, integer LDS atomics, non-zero counters added with 64-bit global atomics).  No
 * floating point, no float atomics: two calls give the same bytes.  Stats: "targeting_units", "targeting_batches", "targeting_us" (host
 * clock).
 *
 * vdjx_targeting_model (plain C, no GPU, no context): the counts -> weights.  obs and opp are the counts of class 0 (cls 0: silent only,
 * shazam's default, so that the model is free of the selection it is used to measure) or of classes 0 + 1 (cls 1).  c: m's centre base.
 *   substitution  a[x] = obs[m][x] (level 5), summed over the 16 5-mers with m's inner three bases (level 3), over the 256 with m's centre
 *                 (level 1): the first level with sum a >= min_sub; otherwise level 0, a[x] = 1 for x != c.  S[x] = a[x] / sum a.
 *   mutability    (o, p) = (sum over x of obs, of opp) at level 5, 3 or 1: the first level with o >= min_mut and p > 0; otherwise level 0,
 *                 all 1,024 5-mers together.  M = o / p; if the level-0 o or p is 0, M = 1 for every 5-mer.
 *   weights       Z = sum M[m], m = 0 .. 1023 in that order; T = (M[m] / Z) * S[x]; weight[m][x] = max(1, rint(T * 1e9)) for x != c and 0
 *                 for x = c: no 5-mer has a zero row.  float64, one operation per statement.  out_level[m] = {substitution level,
 *                 mutability level}.
 * min_sub and min_mut are shazam's minNumMutations (50) and minNumSeqMutations (500).  VDJX_EINVAL: cls outside 0, 1; a minimum of 0; a
 * NULL argument.
 * NOT modelled: shazam's per-sequence normalisation of the background; its N-extended 5-mers; the multipleMutation choice (each differing
 * base is independent here); the clonal consensus sequence (vdjx_consensus, below, is not read here) -- a clone contributes the
 * UNION of its members' events, which is clone-aware already. */
typedef struct { uint64_t contigs, used, truncated, units, positions, obs_s, obs_r, opp_s, opp_r; uint32_t batches, pad; } vdjx_tgt_info;   /* 80 bytes */
int vdjx_targeting_counts(vdjx_ctx* ctx, const char* contigs, size_t n, int len, const vdjx_annot_hit* v, const int32_t* limit,
                          const int32_t* group /* NULL, or n; < 0: no group */, uint64_t* out /* [2][2][1024][4] */, vdjx_tgt_info* info);
int vdjx_targeting_model(const uint64_t* counts /* [2][2][1024][4] */, int cls /* 0: silent only, 1: silent + replacement */,
                         uint64_t min_sub, uint64_t min_mut /* both >= 1 */, uint32_t* out_weight /* [1024][4] */, uint8_t* out_level /* [1024][2] */);

/* ---- clonal consensus sequences: one sequence per lineage, decided column by column ----------------------------------------------------
 * gives `vdjer --consensus` what shazam's collapseClones makes of the clones in a second tool: the sequence a lineage's members agree
 * on, laid against the lineage's V record, so that a lineage counts once and one member's error is outvoted.  Everything is integer: the
 * device's results are bitwise the model's (tests/consensus_model.py).
 *   inputs      contigs, n, len, v[n], limit[n] and group[n] exactly as vdjx_targeting_counts takes them (limit == NULL: len; group ==
 *               NULL or a negative entry: a contig on its own; a hit with more than 64 runs is treated as absent, info->truncated).
 *   units       a unit is a group, or a lone contig.  Its RECORD is the V record most of its contigs with a usable hit name, the lowest
 *               record index on a tie; its VOTERS are the contigs whose usable hit names that record; the group's other usable contigs are
 *               off_record and take no part.  A group without a usable hit is no unit.  Units are numbered from 0 in the order of their
 *               first usable contig; out_unit[i] is the voter's unit, -1 for every other contig.
 *   votes       a voter's runs are walked with q = seq_start - 1, p = germ_start - 1 (0-based contig index and record position).  An M
 *               run of L: for t < L with q + t < limit one vote at p + t for the symbol of contig[q + t] (A, C, G, T; anything else: N);
 *               q and p advance by L.  A D run of L: if q < limit, one vote for GAP at each of p .. p + L - 1; p advances by L.  An I run:
 *               its bases below the limit are counted in info->inserted, q advances, there is no column for them.
 *               lo .. hi: the unit's smallest voted position through its largest + 1; a unit nobody voted in has lo = hi = 0.
 *   decision    at every p in lo .. hi - 1, with the counts c[A, C, G, T, N, gap] and cover = their sum: the candidates are A, C, G, T and
 *               gap (N never wins); best = the largest count of a candidate.  cover = 0 (a hole between two voters' ranges) or best = 0:
 *               N.  One candidate at best: that one.  Several: the germline base of p if it is among them, else N.  Then the threshold:
 *               best * den < num * cover gives N.  num / den = 0 / 1 is shazam's mostCommon, 6000 / 10000 (params == NULL) its
 *               thresholdedFreq at minimumFrequency 0.6.
 *   rows        unit u's rows are hi - lo bytes at out_cons / out_germ + off (out_cover, out_best: entries), no terminator: the consensus
 *               row over ACGTN-, the germline row = the record's characters lo .. hi - 1, not ACGT as N; cover and best as above (each may
 *               be NULL).  off ascends in unit order; the sizes come from vdjx_consensus_layout.
 *   units out   group (-1: a lone contig), gene (the record, as given to vdjx_germline_load), members (the voters), off_record, lo, hi, off.
 *   info        (may be NULL; zeroed first) contigs = n; used: the contigs with a usable hit; truncated; off_record; units; columns: the
 *               sum of hi - lo; votes: the sum of cover; inserted; undecided: the N columns with cover > 0; batches; large_units: the units
 *               of more voters than one workgroup takes (255).
 * The result is a function of the MULTISET of votes: the order of the contigs inside a group, the batches and the launch geometry change
 * no byte.
 * vdjx_consensus_layout (plain C, no GPU, no context): out_unit, the units and the two sizes from the hits alone (it cannot know the record
 * set: a gene is taken as given, germ_end up to 2,047).  out_units has room for n units.
 * vdjx_consensus_hits (plain C, no GPU, no context): pseudo-contig u = the consensus row without its '-', padded with N to plen; *out_plen =
 * the longest, at least 1 (out_contigs == NULL: only that).  Its hit: the unit's gene, seq_start 1, seq_end its bases, germ_start /
 * germ_end after the gap columns at either end are trimmed; runs alternating M (maximal stretches of ACGTN) and D (stretches of '-');
 * matches: the M columns equal and ACGT on both sides, mismatches the other M columns, del the gap columns, ins 0, opens the D runs; score =
 * max(1, matches), n_tied 1.  More than 64 runs: n_runs is kept and runs zeroed, as vdjx_annotate does.  A row without a base: gene -1,
 * score 0.  Such hits are consistent by construction: vdjx_mutations, vdjx_selection and vdjx_targeting_counts take them unchanged.
 * NOT modelled: shazam's mostMutated / leastMutated / catchAll methods; ambiguity codes and stochastic tie-breaking; inserted bases; a
 * consensus of the J segment or the junction; CreateGermlines --cloned's choice among tied V calls (the tie goes to the lowest record).
 * VDJX_EINVAL (the message names the contig): vdjx_targeting_counts' list for the contigs, the V hits and the limit; den outside 1 .. 10^6
 * or num outside 0 .. den; NULL out_cons, out_germ, out_units or out_unit; vdjx_consensus_hits: a plen below the longest row or above
 * 4095.  VDJX_ESTATE: no germline set is loaded.  n = 0 returns at once with a zeroed info.  The host checks every hit, orders the voters
 * by unit with one counting sort and cuts the units into batches of whole units of at most VDJX_CONS_CELLS columns (1 .. 2^28, default 2^24,
 * read per call; 24 bytes of counters each, from the context's workspace; a unit of more columns is a batch of its own); any value gives the
 * same bytes.  Per batch one memset and two kernels: k_cons_vote (a wave per voter; a workgroup takes up to 255 consecutive voters of one
 * unit and counts them in LDS in bytes, 16 KB, with 32-bit LDS atomics; plain stores when it holds the whole unit, 32-bit global atomics
 * otherwise; lone voters store their votes directly) and k_cons_decide (a thread per column).  No floating point, no float atomics: two calls
 * give the same bytes.  Stats: "consensus_units", "consensus_batches", "consensus_us" (host clock). */
typedef struct { int num, den; } vdjx_cons_params;                                                              /* 8 bytes */
typedef struct { int32_t group, gene; uint32_t members, off_record; int32_t lo, hi; uint64_t off; } vdjx_cons_unit;   /* 32 bytes */
typedef struct { uint64_t contigs, used, truncated, off_record, units, columns, votes, inserted, undecided; uint32_t batches, large_units; } vdjx_cons_info;   /* 80 bytes */
int vdjx_consensus_layout(const vdjx_annot_hit* v, const int32_t* limit, const int32_t* group, size_t n, int len, int32_t* out_unit,
                          vdjx_cons_unit* out_units /* up to n */, uint64_t* n_units, uint64_t* n_cols);
int vdjx_consensus(vdjx_ctx* ctx, const char* contigs, size_t n, int len, const vdjx_annot_hit* v, const int32_t* limit, const int32_t* group,
                   const vdjx_cons_params* params /* NULL: 6000 / 10000 */, char* out_cons, char* out_germ, uint32_t* out_cover /* NULL ok */,
                   uint32_t* out_best /* NULL ok */, vdjx_cons_unit* out_units, int32_t* out_unit, vdjx_cons_info* info);
int vdjx_consensus_hits(const vdjx_cons_unit* units, size_t U, const char* cons, const char* germ, int plen,
                        char* out_contigs /* U * plen, or NULL: only *out_plen */, vdjx_annot_hit* out_hits, int* out_plen);

/* ---- bootstrap clonal diversity: the Hill curve D(q) of the clone abundances, resampled to a common depth -----------------------------
 * gives `vdjer --diversity` what alakazam's estimateAbundance / alphaDiversity make of the clone table in a second tool: richness, Shannon
 * and Simpson diversity as points of one curve, each with the spread of B bootstrap replicates rarefied to N draws, so that samples of
 * different depth can be compared.  The draws are integer arithmetic: the device's counts are bitwise the model's
 * (tests/diversity_model.py); the Hill numbers are float64.
 *   inputs      weight[C]: the abundance of every clone in any unit (`vdjer`: hundredths of a read pair); a clone of weight 0 is legal
 *               and is never drawn.  params: replicates B, depth N (the draws of a replicate), seed.  q[Q]: the orders.
 *   draw rule   cum[0] = 0, cum[k + 1] = cum[k] + weight[k], W = cum[C].  mix64 is vdjx_tree_support's (mix64(0) = 0xE220A8397B1DCDAF).
 *               Draw i (0 .. N - 1) of replicate r (1 .. B): u = mix64(mix64(seed) + ((uint64_t) r << 32 | i)), the addition wrapping;
 *               t = floor(u * W / 2^64), the high half of the 128-bit product; the draw falls on the clone k with cum[k] <= t <
 *               cum[k + 1] (an upper bound: a clone of zero width is never hit).  counts[r][k]: the draws of replicate r that fell on k.
 *               Check values: seed 1, r 1, W 3: t for i = 0 .. 11 is 0 2 0 2 1 1 1 2 2 2 1 0; seed 0, r 1, i 0, W 2^62: t =
 *               2241935815489788276; weight (1, 3), N 100000, seed 1, r 1: counts (24932, 75068).
 *   Hill        for one count vector, p_k = c_k / N over the c_k > 0.  q == 0.0: the number of such k (exact); q == 1.0:
 *               exp(-sum p ln p); otherwise (sum p^q)^(1 / (1 - q)).  out_d[(r - 1) * Q + j]: replicate r at order q[j].
 *               out_observed[j]: the same with p_k = weight[k] / W, no resampling.  out_mean[j] and out_sd[j] (with n - 1; 0 when B = 1)
 *               over the replicates are summed on the host in replicate order.
 *   counts      out_counts (may be NULL): uint32 [B * C], replicate-major.
 *   info        (may be NULL; zeroed first, every field filled on success) clones = C; weighted: the clones of weight > 0; weight = W;
 *               depth; replicates; batches: the groups of whole replicates the device ran side by side; path: VDJX_DIV_PATH_LDS or
 *               VDJX_DIV_PATH_GLOBAL, where the draws were counted.
 * NOT modelled: alakazam's unseen-species (Chao1) correction of the abundances; the rank-abundance curve with its intervals; grouping by
 * a second field; rarefaction curves over several depths; beta diversity.
 * VDJX_EINVAL: C >= 2^20; W = 0, or W >= 2^63; replicates outside 1 .. 4096; depth outside 1 .. 2^31 - 1; Q outside 1 .. 64; an order
 * that is NaN, below 0 or above 16; an order with 0 < |q - 1| < 1/64 (the exponent 1 / (1 - q) would magnify the sum's rounding without
 * bound there); NULL weight, q, params, out_observed, out_d, out_mean or out_sd.  C = 0 returns at once with a zeroed info.
 * The host sums the weights; a batch is max(1, floor(cells / C)) whole replicates (cells = VDJX_DIV_CELLS, 1 .. 2^30, the default 2^28
 * counters) and costs one memset and three dispatches (draw, Hill partials, Hill numbers) whatever B, C and N are.  A draw workgroup
 * counts in LDS when C <= VDJX_DIV_LDS_CLONES (0 .. 16384, the default 16384; 0: never) and flushes its non-zero bins with one atomicAdd
 * each, otherwise it adds to global memory directly: integer adds either way, the counts do not depend on their order.  The device's
 * float sums are stored per workgroup and added in a fixed order, no float atomics: two calls give the same bits.  Per batch only its
 * rows of out_d and, if asked for, of out_counts come back.  Stats: "diversity_batches", "diversity_us" (host clock). */
#define VDJX_DIV_PATH_LDS    1
#define VDJX_DIV_PATH_GLOBAL 2
typedef struct { uint32_t replicates, depth; uint64_t seed; } vdjx_diversity_params;                                /* 16 bytes */
typedef struct { uint32_t clones, weighted; uint64_t weight; uint32_t depth, replicates, batches, path; } vdjx_diversity_info;   /* 32 bytes */
int vdjx_diversity(vdjx_ctx* ctx, const uint64_t* weight, size_t C, const double* q, size_t Q, const vdjx_diversity_params* params,
                   double* out_observed, double* out_d, double* out_mean, double* out_sd, uint32_t* out_counts, vdjx_diversity_info* info);

/* rows of `row` bytes on the device: row d_pos[i] of d_dst = row i of d_src.  (The records of a pool sharded by pair on their way to
 * the ranks that hold their slice of the scan order for the k-mer build, A2:1388-1390: every record arrives with its place.) */
int vdjx_rows_scatter(vdjx_ctx* ctx, void* d_dst, const void* d_src, const uint32_t* d_pos, size_t n, size_t row);

/* For the test suite only: the exclusive prefix sum every stage of the device code shares (csrc/vdjx_scan.h), on its own.
 * host_out[i] = host_in[0] + ... + host_in[i - 1] for i = 0 .. n (n + 1 elements of 4 bytes, or of 8 if out_is_u64; 4-byte sums wrap);
 * launches: 1 = one workgroup, 3 = the device-wide form.  VDJX_EINVAL: n >= 2^31, launches neither 1 nor 3. */
int vdjx_scan_u32(vdjx_ctx* ctx, const uint32_t* host_in, size_t n, int out_is_u64, int launches, void* host_out);

/* For the test suite only: the LDS-staged partition pass of the k-mer build (csrc/vdjx_part.h), on its own.  n elements of elem_bytes
 * (8 or 16) go to host_out grouped by bucket, host_starts[0 .. nb] are the buckets' starts (their exclusive prefix sum); the order inside
 * a bucket is arbitrary.  The bucket of an element is bits 40..63 of its first 8-byte word.  An 8-byte element of all ones is a hole:
 * it is dropped, so host_out receives host_starts[nb] <= n elements.  levels 1: nb <= 1024 buckets in one pass, the input shared by
 * `workgroups`.  levels 2: nb = coarse << fine_bits (coarse <= 1024, fine_bits <= 10), the first pass into `coarse` segments, the second
 * inside every segment with `slices` workgroups.  VDJX_EINVAL: elem_bytes, levels, nb or fine_bits outside that, slices or workgroups
 * zero (or above 1024 / 65536), an element whose bucket is not below nb, n >= 2^31. */
int vdjx_part_u64(vdjx_ctx* ctx, const void* host_in, size_t n, int elem_bytes, uint32_t nb, int levels, uint32_t fine_bits, uint32_t slices,
                  uint32_t workgroups, uint32_t* host_starts, void* host_out);

/* counters of the most recent scorer calls, by name: "window_hits" (read instances matched by the last
 * vdjx_window_score call, summed over windows), "window_hits_max", "window_pairs", "window_work_items",
 * "map_hits", "root_dp_items" (and how many of them each DP kernel took: "root_dp_items_wave", one wave per item, and
 * "root_dp_items_thread", one thread per item; they add up to root_dp_items, both 0 where no DP runs).  Unknown names return 0.  Used by bench.py to price the scorers' algorithmic bytes.  vdjx_quant's last
 * call: "quant_map_us", "quant_setup_us", "quant_em_us" (host clock, each phase ending in a wait for the device), "quant_contigs_placed".
 * vdjx_annotate's last call: "annot_cells" (DP cells of the scoring phase), "annot_score_us", "annot_trace_us", "annot_cigar_truncated".
 * vdjx_isotype's last call: "iso_cells" (DP cells of the scoring phase), "iso_score_us", "iso_trace_us" (host clock, each ending in a wait).
 * vdjx_dcall's last call: "dcall_cells" (the sum of win_len times the sum of the records' lengths), "dcall_score_us", "dcall_trace_us".
 * How the last call of each of the three was cut up (0 after a call that failed or had no contig): "annot_chunks", "iso_chunks",
 * "dcall_chunks" (the chunks of the record set, all classes), "annot_score_launches", "iso_score_launches", "dcall_score_launches" (the
 * scoring launches that held work) and "annot_trace_launches", "iso_trace_launches", "dcall_trace_launches" (the traceback launches: 0
 * where no hit was traced, more than 1 where the direction bytes of the hits exceed one launch's).
 * vdjx_mutations' last call: "mutations_cols" (the bytes of each of the three row buffers), "mutations_us" (host clock).
 * vdjx_selection's last call: "selection_chunks" (the partial sums of its large rows), "selection_us" (host clock).
 * vdjx_selection_convolve's last call: "selconv_combines", "selconv_batches", "selconv_us" (host clock).
 * vdjx_diversity's last call: "diversity_batches", "diversity_us" (host clock).
 * vdjx_targeting_counts' last call: "targeting_units", "targeting_batches", "targeting_us" (host clock).
 * vdjx_consensus' last call: "consensus_units", "consensus_batches", "consensus_us" (host clock).
 * What the context keeps from call to call outside its workspaces (anchor bitmaps, V region, read index, the scorers' result and SAM
 * buffers, upload staging, germline / constant / D sets), counted when asked: "kept_device_bytes", "kept_pinned_bytes" (page-locked host
 * memory) and "kept_allocs" (allocations made for them since vdjx_init: unchanged by a call that fitted what was there).  vdjx_trim
 * and vdjx_read_index_drop lower the byte counts.  Defined while no begun read-index build is in flight (it grows the index's arrays
 * on a thread of its own). */
uint64_t vdjx_stat(vdjx_ctx* ctx, const char* name);

/* ---- profiling hooks (HIP events on the context's stream) ---------------------------------------*/
int vdjx_profile_enable(vdjx_ctx* ctx, int on);
/* bracket only the launches of this scope name from now on (NULL: all again): two event records per scope and step cost a small pool's
 * step a tenth of its time; a caller that wants one kernel's duration from inside a region it times pays for that one */
int vdjx_profile_only(vdjx_ctx* ctx, const char* name);
int vdjx_profile_reset(vdjx_ctx* ctx);
/* number of distinct kernel names recorded since the last reset */
int vdjx_profile_count(vdjx_ctx* ctx);
/* idx-th entry: kernel name, summed milliseconds, launch count */
int vdjx_profile_get(vdjx_ctx* ctx, int idx, const char** name, double* total_ms, uint64_t* launches);

/* ---- multi-GPU k-mer build: hash-prefix sharding, partial aggregates merged by the owner ----
 * The reference has no counterpart (its only parallelism is pthreads over roots, A2:1287-1348); these
 * phases split vdjx_kmer_build so that the caller can move the bytes between ranks (one process per GPU;
 * vdjer_amd/shard.py does it with torch.distributed over RCCL, vdjer_amd/csrc/host/vdjx_mgpu.c with RCCL
 * directly).  Record numbering is rank-major with a common stride: rank r's records are
 * [r*rec_stride, r*rec_stride + R_r); instance ids are global, record << 6 | offset, so nranks * rec_stride
 * must stay below 2^32 records (record << 8 | offset and 2^30 records with reads of more than 64 bases).  Any 1 <= nranks <= 256; the owner of a k-mer is its hash bucket divided by
 * the buckets per owner (*dir_len of vdjx_shard_local: the quotient of the bucket count by nranks, rounded up).
 *   Every rank first aggregates ITS OWN gated instances per distinct k-mer (count, first instance, whether it
 * saw two different reads: add_to_table A2:322-367 restated per rank).  These partial aggregates (32 B per
 * distinct gated k-mer per rank, not per instance) are the one bulk exchange.  The owner merges them (counts
 * add, firsts take the minimum, flags OR) and decides almost every k-mer on the spot; only a k-mer whose
 * verdict needs per-read data -- no rank saw two different reads although several hold it, or its count is
 * below the level where the quality sums cannot fail -- costs a question to the ranks that hold it and a
 * fixed-size answer (the first record's bases, partial quality sums).  add_to_graph's bookkeeping (node
 * frequency, first sights of nodes and edges, A2:261-320) is computed by every rank over its own records for
 * ALL survivors and reduced: SUM for the counts, MIN for the first sights.
 * All pointers are device pointers owned by the caller.  Call order (brackets = the caller's collectives):
 *   begin -> (count, symmetric -> [all_reduce MAX, MIN] -> geometry2 ->) local -> local_fill -> [all_to_all: directories, counts, partial aggregates] -> merge
 *   -> queries -> [all_to_all: counts, questions] -> reply -> [all_to_all: answers] -> resolve
 *   -> survivors -> [all_gather] -> edges -> [all_reduce MIN, SUM] -> finish -> free                */
typedef struct vdjx_shard vdjx_shard;
int vdjx_shard_begin(vdjx_ctx* ctx, const vdjx_pool* pool, int k, int mf, int mq, int rank, int nranks,
                     uint64_t rec_stride, vdjx_shard** out);
/* The same build over a SHARE of the pool (the way `vdjer --gpus N` deals the reads: by pair, both mates on one rank): record i of
 * `pool` is record d_scan_index[i] of the scan order of the whole pool (primary then secondary, A2:1388-1390; total_records records
 * over all ranks).  The positions ascend -- a share keeps the pool's order -- and every position belongs to exactly one rank.  The
 * kernels work on local record numbers; a first instance is translated through d_scan_index where it leaves the rank, so no record
 * ever moves between ranks.  d_scan_index is a device pointer that must stay valid until vdjx_shard_free. */
int vdjx_shard_begin_share(vdjx_ctx* ctx, const vdjx_pool* pool, int k, int mf, int mq, int rank, int nranks,
                           const uint32_t* d_scan_index, uint64_t total_records, vdjx_shard** out);
void vdjx_shard_free(vdjx_shard* s);
/* bytes per exchanged record: kind 0 partial aggregate (32), 1 question (8), 2 answer (408: 240 for the k-mer -- the holder's first record,
 * its quality rows -- and, for builds over couples, 168 more for its reverse complement's; always ask, never assume), 3 survivor (32) */
size_t vdjx_shard_record_bytes(int kind);
/* optional, before vdjx_shard_local: this rank's gated k-mer instances (A2:240-259); the ranks compare them [all_reduce MAX] and pass
 * the largest to vdjx_shard_geometry, so that every rank cuts the hash buckets the one-GPU build would cut for the largest rank.
 * Without it the bucket count follows a bound from rec_stride (more, smaller buckets: a partition level more at 10 M pairs per rank). */
int vdjx_shard_count(vdjx_shard* s, uint64_t* gated_instances);
int vdjx_shard_geometry(vdjx_shard* s, uint64_t agreed_instances);
/* A pool as add_to_buffer writes it (bam_read.c:206-244) is made of couples: every read followed by its reverse complement with reversed
 * qualities.  The gated k-mer instances of the second record mirror those of the first, so the local phase can move ONE tuple per pair
 * of mirrored instances -- under the smaller of the k-mer and its reverse complement (k odd) -- and hand both aggregates to the same
 * owner.  That changes which bucket a k-mer falls into, so ALL ranks must do it or none: vdjx_shard_symmetric says whether this rank
 * could (its pool passed the packing's check, k is odd, reads of up to 64 bases); the caller ANDs the ranks' answers [all_reduce MIN]
 * and passes the result to vdjx_shard_geometry2 beside the agreed instance count.  (vdjx_shard_geometry = all_symmetric 0.) */
int vdjx_shard_symmetric(const vdjx_shard* s);
int vdjx_shard_geometry2(vdjx_shard* s, uint64_t agreed_instances, int all_symmetric);
/* this rank's partial aggregates, grouped by owner: send_counts[nranks]; *dir_len = hash buckets per owner */
int vdjx_shard_local(vdjx_shard* s, uint64_t* send_counts, uint32_t* dir_len);
/* d_dir: u32 [nranks*dir_len] partial aggregates per bucket (owner-major); d_partials: sum(send_counts) records, 16-byte aligned.
 * The aggregates are laid end to end IN d_partials, which must stay valid and unchanged until vdjx_shard_reply has returned (the
 * answers to the owners' questions are looked up in it: no second copy of a gigabyte per rank). */
int vdjx_shard_local_fill(vdjx_shard* s, void* d_dir, void* d_partials);
/* owner: directories and partial aggregates as received (source-major) -> decided k-mers and questions;
 * query_counts[r] = questions for rank r */
int vdjx_shard_merge(vdjx_shard* s, const void* d_recv_dir, const void* d_recv_partials, const uint64_t* recv_counts,
                     uint64_t* query_counts);
/* the questions, grouped by destination rank: sum(query_counts) records */
int vdjx_shard_queries(vdjx_shard* s, void* d_out);
/* every rank: the questions it received (counts[o] from owner o, in that order) -> answers in the same order */
int vdjx_shard_reply(vdjx_shard* s, const void* d_queries, const uint64_t* counts, void* d_replies);
/* owner: the answers (grouped by answering rank, each group in question order) -> this rank's survivors
 * (a-1/a-2 for the k-mers it owns); n_distinct = distinct gated k-mers it owns ("Pre Num nodes") */
int vdjx_shard_resolve(vdjx_shard* s, const void* d_replies, uint64_t n_replies, uint64_t* n_survivors, uint64_t* n_distinct);
/* n_survivors records of 32 B: {u64 key_lo, u64 key_hi, u32 gated count, u32 -, u64 first gated instance} */
int vdjx_shard_survivors(vdjx_shard* s, void* d_out);
/* all ranks' survivors (rank order) -> this rank's share of add_to_graph (A2:261-320) over ITS records:
 * d_in_first u64 [ns_total*4]: first sight (global instance id, all-ones = none) of the edge into survivor v whose tail
 * k-mer starts with base a, at [v*4+a]; d_ufirst u64 [ns_total]: first sight of the node; d_ucnt u32 [ns_total]:
 * its instances on this rank.  The caller reduces over ranks: MIN (unsigned order) for d_in_first and d_ufirst,
 * SUM for d_ucnt */
int vdjx_shard_edges(vdjx_shard* s, const void* d_surv_all, uint64_t ns_total, void* d_in_first, void* d_ucnt, void* d_ufirst);
/* reduced arrays -> the graph, identical on every rank */
int vdjx_shard_finish(vdjx_shard* s, const void* d_in_first, const void* d_ucnt, const void* d_ufirst,
                      uint64_t pre_nodes_total, vdjx_graph** out);

#ifdef __cplusplus
}
#endif
#endif
