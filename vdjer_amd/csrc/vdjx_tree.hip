// vdjx_tree.hip -- lineage trees: the minimum spanning tree of every clone under the Hamming distance of its members' common window
// (gfx950 only, wave64).
//
//   vdjx_tree   the members of a clone are compared all against all over the window around their anchors; Boruvka's rounds pick, per
//               component, the smallest edge that leaves it (the model: include/vdjx.h; in Python: tests/tree_model.py)
//
// The host sorts the (clone, index) keys -- per item --, computes each clone's window and lays the members out in clone order ("rows":
// vdjx_treelay.h).
// Inside a clone the rows are in index order, so the order of two rows is the order of the caller's indices: the edge keys carry ROW
// numbers and compare as the model's (d, min(i, j), max(i, j)) do.  Per pair everything happens on the device, in 1 + 3 * rounds
// dispatches, rounds = ceil(log2(largest clone)), whatever n and the number of clones are; nothing is read back between the rounds:
//   k_tree_pack   a row = `words` {bases, mask} pairs in vdjx_hamming.h's format, bits past the window 0.  The window is cut out of the
//                 contig at the member's own offset, character by character: any shift.  comp[r] = parent[r] = r.
//   k_tree_min    one wave per work item (row block of 64 rows, column slice of the same clone).  Up to 16 words (512 bases) a lane keeps
//                 its row in registers and the columns go through LDS in tiles, read back as one 16-byte broadcast per word (ham_word);
//                 wider windows walk the words in chunks of 16 against tiles of 8 columns, a running d per column.  Against every column of another
//                 component the lane forms d << 40 | lo << 20 | hi and keeps the smallest; one atomicMin per lane on best[comp[row]]
//                 at the end (a minimum: the order it lands in does not matter).
//   k_tree_hook   per component with a best edge: the edge is appended (once: where both ends chose it, the smaller root does) and
//                 its two ends are united in parent[] (vdjx_unionfind.h: the larger root goes under the smaller).  comp[] -- the
//                 components this round began with -- is only read.
//   k_tree_flat   comp[r] = the root of r in parent[]; best[r] = none.
// The keys are distinct, so the chosen edges never close a cycle and the components at least halve per round.  The edges (members -
// clones) come back once, in whatever order the appends landed; the host orients them toward each clone's root and counts the depths,
// O(n), which does not depend on that order.  No floating point.  Scratch comes from the context's workspace.
//
//   vdjx_tree_support   the delete-half jackknife: every replicate keeps about half of the window's columns and builds the trees again
//               on the kept columns alone; an edge's support is the number of replicates whose tree has it.  The rounds are the same
//               routine (tree_rounds) on other rows:
//   k_tree_pack_sel   as k_tree_pack, but a row's characters are gathered at the replicate's kept positions (a list per replicate, made
//                 on the host), so a replicate's rows have about half the words and k_tree_min runs on them as it is.  A batch is as
//                 many whole replicates side by side as fit below 2^20 rows (VDJX_TREE_SUPPORT_ROWS), replicate-major, each
//                 (replicate, clone) a clone of its own to the rounds.
//   k_tree_support    per edge of the batch's trees: the two rows back to the caller's items, one atomicAdd on the end whose scored parent
//                 is the other.  Per batch only the edge count is read back; the supports once, at the end.
#include "vdjx_common.h"
#include "vdjx_hamming.h"
#include "vdjx_treelay.h"
#include "vdjx_unionfind.h"

#include <string.h>

#define TREE_NONE 0xFFFFFFFFFFFFFFFFull
#define TREE_REG_WORDS 16                // a row of up to 16 words (512 bases) stays in registers
#define TREE_LDS 512u                    // {bases, mask} pairs of a tile: 8 KiB, 64 columns of up to 8 words or 32 of up to 16
#define TREE_CH_COLS 8                   // the chunked path: columns per tile, each with a running distance in a register

// the user words of a clone's work items: u[0] the clone's first row, u[1] its first word

// one thread per {bases, mask} pair; ri[rows] is a sentinel whose wbase is the number of pairs.  SEL is the jackknife's pack: a row's
// characters are the replicate's kept window positions (sel: `stride` ascending positions per replicate of the batch, of which the row
// uses its first q.w); the rows of a replicate are `per_rep` in a run
template <bool SEL>
__global__ __launch_bounds__(256) void k_tree_pack(const char* __restrict__ contigs, const TreeRow* __restrict__ ri, u32 rows, u32 total,
                                                   const uint16_t* __restrict__ sel, u32 stride, u32 per_rep, ulonglong2* __restrict__ out,
                                                   u32* __restrict__ comp, u32* __restrict__ parent, unsigned long long* __restrict__ best) {
	const u32 t = blockIdx.x * 256u + threadIdx.x;
	if (t >= total) return;
	u32 lo = 0, hi = rows;                              // the row r with ri[r].wbase <= t < ri[r + 1].wbase
	while (hi - lo > 1u) {
		const u32 mid = (lo + hi) / 2u;
		if (ri[mid].wbase <= t) lo = mid; else hi = mid;
	}
	const TreeRow q = ri[lo];
	const u32 w = t - q.wbase;
	const uint16_t* mine = SEL ? sel + (size_t) (lo / per_rep) * stride : nullptr;
	// (a replicate that keeps nothing of this window: one word of zeros)
	out[t] = ham_pack_word([&](u32 pos) { return contigs[q.at + (SEL ? mine[pos] : pos)]; }, w, q.w);
	if (w == 0) { comp[lo] = lo; parent[lo] = lo; best[lo] = TREE_NONE; }
}

__device__ inline u64 tree_key(u32 d, u32 a, u32 b) { return (u64) d << 40 | (u64) (a < b ? a : b) << 20 | (u64) (a < b ? b : a); }

// the register path: W words per row, tiles of TREE_LDS / W columns (a power of two of them)
template <int W>
__device__ inline void tree_item(const HamItem it, const ulonglong2* __restrict__ words, const u32* __restrict__ comp, unsigned long long* best,
                                 ulonglong2* tile, u32* tile_comp) {
	constexpr u32 TC = W <= 8 ? 64u : 32u;
	const u32 lane = threadIdx.x, myrow = it.row0 + lane;
	const bool live = myrow < it.row_end;
	const u32 r = live ? myrow : it.row0;
	const ulonglong2* cw = words + it.u[1];              // the clone's rows, W pairs each
	u64 x[W], m[W];
#pragma unroll
	for (int w = 0; w < W; w++) {
		const ulonglong2 q = cw[(size_t) (r - it.u[0]) * W + w];
		x[w] = q.x;
		m[w] = q.y;
	}
	const u32 mine = comp[r];
	u64 bk = TREE_NONE;
	for (u32 base = it.col0; base < it.col_end; base += TC) {
		const u32 nc = min(TC, it.col_end - base);
		const ulonglong2* src = cw + (size_t) (base - it.u[0]) * W;      // (the tile's columns are contiguous)
		for (u32 i = lane; i < nc * (u32) W; i += 64u) tile[i] = src[i];
		if (lane < nc) tile_comp[lane] = comp[base + lane];
		__syncthreads();
		for (u32 c = 0; c < nc; c++) {
			const bool other = live && tile_comp[c] != mine;
			if (!__any(other)) continue;                   // (wave-uniform: a column of every lane's own component)
			u32 d = 0;
#pragma unroll
			for (int w = 0; w < W; w++) d += ham_word(x[w], m[w], tile[c * (u32) W + w]);   // (every lane the same address: one broadcast read of 16 bytes)
			if (other) {
				const u64 k = tree_key(d, myrow, base + c);
				bk = k < bk ? k : bk;
			}
		}
		__syncthreads();
	}
	if (live && bk != TREE_NONE) atomicMin(best + mine, (unsigned long long) bk);
}

// the chunked path: any number of words.  Per tile of 8 columns the words go by in chunks of 16: the lane's chunk in registers, the
// columns' in LDS, a running distance per column.  Words past the row's end count as 0 on both sides.
__device__ inline void tree_item_wide(const HamItem it, const ulonglong2* __restrict__ words, const u32* __restrict__ comp, unsigned long long* best,
                                      ulonglong2* tile, u32* tile_comp) {
	const u32 lane = threadIdx.x, myrow = it.row0 + lane, W = it.words, first = it.u[0];
	const bool live = myrow < it.row_end;
	const u32 r = live ? myrow : it.row0;
	const ulonglong2* cw = words + it.u[1];
	const ulonglong2* mw = cw + (size_t) (r - first) * W;
	const u32 mine = comp[r];
	u64 bk = TREE_NONE;
	for (u32 base = it.col0; base < it.col_end; base += TREE_CH_COLS) {
		const u32 nc = min((u32) TREE_CH_COLS, it.col_end - base);
		u32 d[TREE_CH_COLS];
#pragma unroll
		for (int c = 0; c < TREE_CH_COLS; c++) d[c] = 0;
		if (lane < nc) tile_comp[lane] = comp[base + lane];
		for (u32 w0 = 0; w0 < W; w0 += TREE_REG_WORDS) {
			u64 x[TREE_REG_WORDS], m[TREE_REG_WORDS];
#pragma unroll
			for (int w = 0; w < TREE_REG_WORDS; w++) {
				const ulonglong2 q = w0 + (u32) w < W ? mw[w0 + (u32) w] : make_ulonglong2(0, 0);
				x[w] = q.x;
				m[w] = q.y;
			}
			for (u32 i = lane; i < TREE_CH_COLS * TREE_REG_WORDS; i += 64u) {
				const u32 c = i / TREE_REG_WORDS, w = w0 + i % TREE_REG_WORDS;
				tile[i] = c < nc && w < W ? cw[(size_t) (base + c - first) * W + w] : make_ulonglong2(0, 0);
			}
			__syncthreads();
#pragma unroll
			for (int c = 0; c < TREE_CH_COLS; c++)
#pragma unroll
				for (int w = 0; w < TREE_REG_WORDS; w++) d[c] += ham_word(x[w], m[w], tile[c * TREE_REG_WORDS + w]);
			__syncthreads();
		}
#pragma unroll
		for (int c = 0; c < TREE_CH_COLS; c++)
			if ((u32) c < nc && live && tile_comp[c] != mine) {
				const u64 k = tree_key(d[c], myrow, base + (u32) c);
				bk = k < bk ? k : bk;
			}
		__syncthreads();                                    // (tile_comp is written again at the top)
	}
	if (live && bk != TREE_NONE) atomicMin(best + mine, (unsigned long long) bk);
}

// one wave per work item; the word count is the clone's, so it is uniform and every loop over words is unrolled
__global__ __launch_bounds__(64) void k_tree_min(const HamItem* __restrict__ items, const ulonglong2* __restrict__ words, const u32* __restrict__ comp,
                                                 unsigned long long* best) {
	__shared__ ulonglong2 tile[TREE_LDS];
	__shared__ u32 tile_comp[64];
	const HamItem it = items[blockIdx.x];
	switch (it.words) {                                    // (W below is the case's constant: HAM_CASES_16 declares it)
		HAM_CASES_16(tree_item<W>(it, words, comp, best, tile, tile_comp))
		default: tree_item_wide(it, words, comp, best, tile, tile_comp); break;
	}
}

// one thread per row; only the roots of the round's components act
__global__ __launch_bounds__(256) void k_tree_hook(const u32* __restrict__ comp, const unsigned long long* __restrict__ best, u32 rows, u32* parent,
                                                   unsigned long long* __restrict__ edges, u32 cap, u32* n_edges) {
	const u32 r = blockIdx.x * 256u + threadIdx.x;
	if (r >= rows || comp[r] != r) return;
	const u64 k = best[r];
	if (k == TREE_NONE) return;
	const u32 lo = (u32) (k >> 20) & 0xFFFFFu, hi = (u32) k & 0xFFFFFu;
	if (lo >= rows || hi >= rows) return;                 // (cannot be: k_tree_min made the key of two rows)
	const u32 ca = comp[lo], cb = comp[hi], other = ca == r ? cb : ca;
	if (best[other] == k && other < r) return;            // both ends chose this edge: the smaller root appends and unites
	const u32 slot = atomicAdd(n_edges, 1u);
	if (slot < cap) edges[slot] = k;
	uf_unite(parent, lo, hi);
}

__global__ __launch_bounds__(256) void k_tree_flat(const u32* __restrict__ parent, u32 rows, u32* __restrict__ comp, unsigned long long* __restrict__ best) {
	const u32 r = blockIdx.x * 256u + threadIdx.x;
	if (r >= rows) return;
	u32 x = parent[r];
	for (u32 p = parent[x]; p != x; p = parent[x]) x = p;
	comp[r] = x;
	best[r] = TREE_NONE;
}

// one thread per edge of the batch's replicate trees: row r is member r % per_rep of its replicate, item[] the caller's index of a member.
// The edge {i, j} counts for the end whose scored parent is the other (a sum: the order of the atomics does not matter)
__global__ __launch_bounds__(256) void k_tree_support(const unsigned long long* __restrict__ edges, const u32* __restrict__ n_edges, u32 cap, u32 rows,
                                                      u32 per_rep, const u32* __restrict__ item, const int32_t* __restrict__ parent, u32* support) {
	const u32 e = blockIdx.x * 256u + threadIdx.x;
	if (e >= cap || e >= *n_edges) return;
	const u64 k = edges[e];
	const u32 lo = (u32) (k >> 20) & 0xFFFFFu, hi = (u32) k & 0xFFFFFu;
	if (lo >= rows || hi >= rows) return;                 // (cannot be: k_tree_min made the key of two rows)
	const u32 i = item[lo % per_rep], j = item[hi % per_rep];
	if (parent[i] == (int32_t) j) atomicAdd(support + i, 1u);
	if (parent[j] == (int32_t) i) atomicAdd(support + j, 1u);
}

// Boruvka's rounds over laid-out rows (packed, comp = parent = the row, best = none): per round min, hook, flat; nothing is read back
static void tree_rounds(vdjx_ctx* c, hipStream_t st, u32 rounds, const HamItem* d_items, u32 n_items, const ulonglong2* d_words, u32 rows, u32* d_comp,
                        u32* d_parent, unsigned long long* d_best, unsigned long long* d_edges, u32 cap, u32* d_count) {
	const u32 nb = (rows + 255u) / 256u;
	for (u32 round = 0; round < rounds; round++) {
		{
			vdjx_prof_scope ps(c, round ? "k_tree_min" : "k_tree_min_first");      // (the first round skips no column: the pass to measure)
			hipLaunchKernelGGL(k_tree_min, dim3(n_items), dim3(64), 0, st, d_items, d_words, (const u32*) d_comp, d_best);
		}
		{
			vdjx_prof_scope ps(c, "k_tree_hook");
			hipLaunchKernelGGL(k_tree_hook, dim3(nb), dim3(256), 0, st, (const u32*) d_comp, (const unsigned long long*) d_best, rows, d_parent, d_edges, cap,
			                   d_count);
		}
		{
			vdjx_prof_scope ps(c, "k_tree_flat");
			hipLaunchKernelGGL(k_tree_flat, dim3(nb), dim3(256), 0, st, (const u32*) d_parent, rows, d_comp, d_best);
		}
	}
}

extern "C" int vdjx_tree(vdjx_ctx* c, const char* contigs, size_t n, int len, const int32_t* clone, const int32_t* anchor, const uint32_t* prio,
                         int32_t* out_parent, int32_t* out_dist, int32_t* out_depth, vdjx_tree_info* info) {
	if (info) memset(info, 0, sizeof *info);
	if (!c) { vdjx_set_error("vdjx_tree: NULL argument"); return VDJX_EINVAL; }
	if (n == 0) return VDJX_OK;
	if (!contigs || !clone || !anchor || !out_parent || !out_dist || !out_depth) { vdjx_set_error("vdjx_tree: NULL argument"); return VDJX_EINVAL; }
	if (int rc = tree_check_contigs("vdjx_tree", contigs, n, len)) return rc;
	const auto t0 = std::chrono::steady_clock::now();
	std::vector<u64> keys;
	if (int rc = tree_keys("vdjx_tree", n, len, clone, anchor, keys)) return rc;
	const u32 rows = (u32) keys.size();
	for (size_t i = 0; i < n; i++) out_parent[i] = out_dist[i] = out_depth[i] = -1;
	vdjx_tree_info inf;
	memset(&inf, 0, sizeof inf);
	inf.members = rows;
	if (rows == 0) {
		if (info) *info = inf;
		c->stats["tree_work_items"] = 0;
		c->stats["tree_rounds"] = 0;
		c->stats["tree_us"] = 0;
		return VDJX_OK;
	}
	TreeLay L;
	if (int rc = tree_lay("vdjx_tree", keys, len, clone, anchor, prio, L)) return rc;
	const std::vector<TreeClone>& clones = L.clones;
	const std::vector<TreeRow>& ri = L.ri;
	const std::vector<u32>& row_item = L.row_item;
	const u64 total = L.total;
	inf.largest_clone = L.largest;
	inf.clones = (u32) clones.size();
	inf.edges = (u64) rows - clones.size();
	while ((1ull << inf.rounds) < inf.largest_clone) inf.rounds++;
	const u32 slice = ham_slice_width(L.cells);
	std::vector<HamItem> items;                            // a clone of two and more is a group (a clone of one has no item)
	for (const TreeClone& q : clones)
		if (q.m >= 2) ham_slice_items({q.first, q.m, q.words, {q.first, q.wbase, 0u}}, slice, items);
	const u32 cap = (u32) inf.edges;
	std::vector<u64> edges(cap ? cap : 1);
	u32 n_edges = 0;
	if (inf.rounds) {
		HIP_TRY(hipSetDevice(c->device));
		hipStream_t st = c->stream;
		vdjx_work wk(c);
		char* d_contigs;
		TreeRow* d_ri;
		HamItem* d_items;
		ulonglong2* d_words;
		u32 *d_comp, *d_parent, *d_count;
		unsigned long long *d_best, *d_edges;
		HIP_TRY(wk.alloc(&d_contigs, n * (size_t) len));
		HIP_TRY(wk.alloc(&d_ri, (size_t) rows + 1));
		HIP_TRY(wk.alloc(&d_items, items.size()));
		HIP_TRY(wk.alloc(&d_words, (size_t) total));
		HIP_TRY(wk.alloc(&d_comp, rows));
		HIP_TRY(wk.alloc(&d_parent, rows));
		HIP_TRY(wk.alloc(&d_best, rows));
		HIP_TRY(wk.alloc(&d_edges, cap));
		HIP_TRY(wk.alloc(&d_count, 1));
		HIP_TRY(hipMemcpyAsync(d_contigs, contigs, n * (size_t) len, hipMemcpyHostToDevice, st));
		HIP_TRY(hipMemcpyAsync(d_ri, ri.data(), ((size_t) rows + 1) * sizeof(TreeRow), hipMemcpyHostToDevice, st));
		HIP_TRY(hipMemcpyAsync(d_items, items.data(), items.size() * sizeof(HamItem), hipMemcpyHostToDevice, st));
		HIP_TRY(hipMemsetAsync(d_count, 0, sizeof(u32), st));
		{
			vdjx_prof_scope ps(c, "k_tree_pack");
			hipLaunchKernelGGL(k_tree_pack<false>, dim3((u32) ((total + 255) / 256)), dim3(256), 0, st, (const char*) d_contigs, (const TreeRow*) d_ri, rows, (u32) total,
			                   (const uint16_t*) nullptr, 0u, 1u, d_words, d_comp, d_parent, d_best);      // (sel, stride, per_rep: not read without SEL)
		}
		tree_rounds(c, st, inf.rounds, d_items, (u32) items.size(), d_words, rows, d_comp, d_parent, d_best, d_edges, cap, d_count);
		HIP_TRY(hipMemcpyAsync(&n_edges, d_count, sizeof n_edges, hipMemcpyDeviceToHost, st));
		HIP_TRY(hipMemcpyAsync(edges.data(), d_edges, (size_t) cap * sizeof(u64), hipMemcpyDeviceToHost, st));
		HIP_TRY(hipStreamSynchronize(st));
		HIP_TRY(hipGetLastError());
		vdjx_prof_collect(c, false);
	}
	if (n_edges != cap) { vdjx_set_error("vdjx_tree: %u edges for %u members in %u clones", n_edges, rows, inf.clones); return VDJX_ESTATE; }
	// the edges toward the roots: adjacency lists over the rows, then a walk from every clone's root
	std::vector<u32> deg(rows + 1, 0), adj(2 * (size_t) cap), adj_d(2 * (size_t) cap);
	for (u32 e = 0; e < cap; e++) {
		const u32 lo = (u32) (edges[e] >> 20) & 0xFFFFFu, hi = (u32) edges[e] & 0xFFFFFu;
		if (lo >= rows || hi >= rows || lo == hi) { vdjx_set_error("vdjx_tree: an edge between rows %u and %u of %u", lo, hi, rows); return VDJX_ESTATE; }
		deg[lo + 1]++;
		deg[hi + 1]++;
	}
	for (u32 r = 0; r < rows; r++) deg[r + 1] += deg[r];
	std::vector<u32> fill(deg.begin(), deg.end() - 1);
	for (u32 e = 0; e < cap; e++) {
		const u32 lo = (u32) (edges[e] >> 20) & 0xFFFFFu, hi = (u32) edges[e] & 0xFFFFFu, d = (u32) (edges[e] >> 40);
		adj[fill[lo]] = hi; adj_d[fill[lo]++] = d;
		adj[fill[hi]] = lo; adj_d[fill[hi]++] = d;
	}
	std::vector<u32> queue(rows);
	u32 reached = 0;
	for (const TreeClone& q : clones) {
		u32 head = reached;
		queue[reached++] = q.root;
		out_depth[row_item[q.root]] = 0;
		while (head < reached) {
			const u32 r = queue[head++], i = row_item[r];
			for (u32 k = deg[r]; k < deg[r + 1]; k++) {
				const u32 s = adj[k], j = row_item[s];
				if (out_depth[j] >= 0) continue;              // (its parent: the only neighbour seen before)
				out_parent[j] = (int32_t) i;
				out_dist[j] = (int32_t) adj_d[k];
				out_depth[j] = out_depth[i] + 1;
				inf.weight += adj_d[k];
				if (reached < rows) queue[reached++] = s;
			}
		}
	}
	if (reached != rows) { vdjx_set_error("vdjx_tree: %u of %u members reached from the roots", reached, rows); return VDJX_ESTATE; }
	if (info) *info = inf;
	c->stats["tree_work_items"] = items.size();
	c->stats["tree_rounds"] = inf.rounds;
	c->stats["tree_us"] = (u64) std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
	return VDJX_OK;
}

// vdjx_tree_support -- the delete-half jackknife over the window's columns.  The host lays the clones of two and more out once ("per
// replicate": member p of M), computes every replicate's kept positions and, per batch of whole replicates, the rows (replicate-major:
// row = replicate * M + p) with their kept counts and the work items; a batch is 1 + 3 * rounds + 1 dispatches: k_tree_pack_sel, the
// rounds of vdjx_tree on rows of about half the words, k_tree_support.  Only the edge count comes back per batch.
extern "C" int vdjx_tree_support(vdjx_ctx* c, const char* contigs, size_t n, int len, const int32_t* clone, const int32_t* anchor, const int32_t* parent,
                                 const vdjx_tree_support_params* params, int32_t* out_support, vdjx_tree_support_info* info) {
	static const char* who = "vdjx_tree_support";
	if (info) memset(info, 0, sizeof *info);
	if (!c) { vdjx_set_error("%s: NULL argument", who); return VDJX_EINVAL; }
	if (n == 0) return VDJX_OK;
	if (!contigs || !clone || !anchor || !params) { vdjx_set_error("%s: NULL argument", who); return VDJX_EINVAL; }
	if (!parent) { vdjx_set_error("%s: NULL argument (parent)", who); return VDJX_EINVAL; }
	if (!out_support) { vdjx_set_error("%s: NULL argument (out_support)", who); return VDJX_EINVAL; }
	if (params->replicates < 1 || params->replicates > 1024) { vdjx_set_error("%s: %u replicates (1 .. 1024)", who, params->replicates); return VDJX_EINVAL; }
	if (int rc = tree_check_contigs(who, contigs, n, len)) return rc;
	const auto t0 = std::chrono::steady_clock::now();
	const u32 B = params->replicates;
	std::vector<u64> keys;
	if (int rc = tree_keys(who, n, len, clone, anchor, keys)) return rc;
	vdjx_tree_support_info inf;
	memset(&inf, 0, sizeof inf);
	for (size_t i = 0; i < n; i++) {
		const int32_t p = parent[i];
		if (p < -1 || (p >= 0 && (size_t) p >= n)) { vdjx_set_error("%s: parent of item %zu is %d (-1 .. %zu)", who, i, p, n - 1); return VDJX_EINVAL; }
		if (p < 0) continue;
		if (clone[i] < 0) { vdjx_set_error("%s: parent of item %zu is %d, but the item is in no clone", who, i, p); return VDJX_EINVAL; }
		if ((size_t) p == i) { vdjx_set_error("%s: parent of item %zu is the item itself", who, i); return VDJX_EINVAL; }
		if (clone[p] != clone[i]) { vdjx_set_error("%s: parent of item %zu is %d, of another clone (%d, not %d)", who, i, p, clone[p], clone[i]); return VDJX_EINVAL; }
		inf.edges++;
	}
	const u32 rows = (u32) keys.size();
	TreeLay L;
	if (rows)
		if (int rc = tree_lay(who, keys, len, clone, anchor, nullptr, L)) return rc;
	for (size_t i = 0; i < n; i++) out_support[i] = parent[i] >= 0 ? 0 : -1;
	inf.members = rows;
	inf.clones = (u32) L.clones.size();
	inf.largest_clone = L.largest;
	inf.replicates = B;
	while ((1ull << inf.rounds) < inf.largest_clone) inf.rounds++;
	// per replicate: the members of the clones of two and more, in row order
	struct Big { u32 first, m, w; };
	std::vector<Big> big;
	std::vector<u32> item;
	std::vector<u64> at;
	u32 maxw = 0;
	for (const TreeClone& q : L.clones) {
		if (q.m < 2) continue;
		big.push_back({(u32) item.size(), q.m, q.w});
		for (u32 r = q.first; r < q.first + q.m; r++) {
			item.push_back(L.row_item[r]);
			at.push_back(L.ri[r].at);
		}
		maxw = std::max(maxw, q.w);
	}
	const u32 M = (u32) item.size(), per_edges = M - (u32) big.size();
	u64 work_items = 0;
	if (M) {
		const u32 row_budget = (u32) vdjx_env_num("VDJX_TREE_SUPPORT_ROWS", (1 << 20) - 1, 1, (1 << 20) - 1);
		const u32 per_batch = std::max(1u, row_budget / M);
		HIP_TRY(hipSetDevice(c->device));
		hipStream_t st = c->stream;
		vdjx_work wk(c);
		char* d_contigs;
		u32 *d_item, *d_support;
		int32_t* d_scored;
		HIP_TRY(wk.alloc(&d_contigs, n * (size_t) len));
		HIP_TRY(wk.alloc(&d_item, M));
		HIP_TRY(wk.alloc(&d_scored, n));
		HIP_TRY(wk.alloc(&d_support, n));
		HIP_TRY(hipMemcpyAsync(d_contigs, contigs, n * (size_t) len, hipMemcpyHostToDevice, st));
		HIP_TRY(hipMemcpyAsync(d_item, item.data(), (size_t) M * sizeof(u32), hipMemcpyHostToDevice, st));
		HIP_TRY(hipMemcpyAsync(d_scored, parent, n * sizeof(int32_t), hipMemcpyHostToDevice, st));
		HIP_TRY(hipMemsetAsync(d_support, 0, n * sizeof(u32), st));
		const vdjx_arena::mark_t mk = wk.mark();
		std::vector<uint16_t> sel;
		std::vector<TreeRow> ri;
		std::vector<HamItem> items;
		u64 rep_cells = 0;                                   // the squared clone sizes of one replicate
		for (const Big& g : big) rep_cells += (u64) g.m * g.m;
		for (u32 r0 = 0; r0 < B; r0 += per_batch) {
			const u32 reps = std::min(per_batch, B - r0), brows = reps * M, cap = reps * per_edges;
			sel.assign((size_t) reps * maxw, 0);
			ri.resize((size_t) brows + 1);
			items.clear();
			const u32 slice = ham_slice_width((u64) reps * rep_cells);
			u64 total = 0;
			for (u32 k = 0; k < reps; k++) {
				const u64 r = (u64) r0 + k + 1;                 // replicates count from 1
				uint16_t* mine = sel.data() + (size_t) k * maxw;
				u32 kept = 0;
				u64 bits = 0;
				for (u32 q = 0; q < maxw; q++) {
					if ((q & 31u) == 0) bits = vdjx_mix64(params->seed ^ (r << 32 | (u64) (q >> 5)));
					if (bits >> (q & 31u) & 1u) mine[kept++] = (uint16_t) q;
				}
				for (const Big& g : big) {
					const u32 kw = (u32) (std::lower_bound(mine, mine + kept, (uint16_t) g.w) - mine);      // kept positions below the clone's w (w < 4096)
					const u32 words = std::max(1u, (kw + 31u) / 32u), first = k * M + g.first;
					if (total + (u64) g.m * words > 0xFFFFFFFFull) { vdjx_set_error("%s: more than 2^32 packed words", who); return VDJX_ELIMIT; }
					for (u32 p = 0; p < g.m; p++) ri[first + p] = {at[g.first + p], (u32) total + p * words, kw};
					ham_slice_items({first, g.m, words, {first, (u32) total, 0u}}, slice, items);      // each (replicate, clone) a group of its own
					total += (u64) g.m * words;
				}
			}
			ri[brows] = {0, (u32) total, 0};
			work_items += items.size();
			uint16_t* d_sel;
			TreeRow* d_ri;
			HamItem* d_items;
			ulonglong2* d_words;
			u32 *d_comp, *d_parent, *d_count;
			unsigned long long *d_best, *d_edges;
			HIP_TRY(wk.alloc(&d_sel, sel.size()));
			HIP_TRY(wk.alloc(&d_ri, (size_t) brows + 1));
			HIP_TRY(wk.alloc(&d_items, items.size()));
			HIP_TRY(wk.alloc(&d_words, (size_t) total));
			HIP_TRY(wk.alloc(&d_comp, brows));
			HIP_TRY(wk.alloc(&d_parent, brows));
			HIP_TRY(wk.alloc(&d_best, brows));
			HIP_TRY(wk.alloc(&d_edges, cap));
			HIP_TRY(wk.alloc(&d_count, 1));
			HIP_TRY(hipMemcpyAsync(d_sel, sel.data(), sel.size() * sizeof(uint16_t), hipMemcpyHostToDevice, st));
			HIP_TRY(hipMemcpyAsync(d_ri, ri.data(), ((size_t) brows + 1) * sizeof(TreeRow), hipMemcpyHostToDevice, st));
			HIP_TRY(hipMemcpyAsync(d_items, items.data(), items.size() * sizeof(HamItem), hipMemcpyHostToDevice, st));
			HIP_TRY(hipMemsetAsync(d_count, 0, sizeof(u32), st));
			{
				vdjx_prof_scope ps(c, "k_tree_pack_sel");
				hipLaunchKernelGGL(k_tree_pack<true>, dim3((u32) ((total + 255) / 256)), dim3(256), 0, st, (const char*) d_contigs, (const TreeRow*) d_ri, brows, (u32) total,
				                   (const uint16_t*) d_sel, maxw, M, d_words, d_comp, d_parent, d_best);
			}
			tree_rounds(c, st, inf.rounds, d_items, (u32) items.size(), d_words, brows, d_comp, d_parent, d_best, d_edges, cap, d_count);
			{
				vdjx_prof_scope ps(c, "k_tree_support");
				hipLaunchKernelGGL(k_tree_support, dim3((cap + 255u) / 256u), dim3(256), 0, st, (const unsigned long long*) d_edges, (const u32*) d_count, cap, brows, M,
				                   (const u32*) d_item, (const int32_t*) d_scored, d_support);
			}
			u32 n_edges = 0;
			HIP_TRY(hipMemcpyAsync(&n_edges, d_count, sizeof n_edges, hipMemcpyDeviceToHost, st));
			HIP_TRY(hipStreamSynchronize(st));
			HIP_TRY(hipGetLastError());
			vdjx_prof_collect(c, false);
			if (n_edges != cap) {
				vdjx_set_error("%s: %u edges for %u members in %zu clones of %u replicates", who, n_edges, M, big.size(), reps);
				return VDJX_ESTATE;
			}
			wk.release_to(mk);
			inf.batches++;
		}
		std::vector<u32> support(n);
		HIP_TRY(hipMemcpyAsync(support.data(), d_support, n * sizeof(u32), hipMemcpyDeviceToHost, st));
		HIP_TRY(hipStreamSynchronize(st));
		for (size_t i = 0; i < n; i++) {
			if (parent[i] < 0) continue;
			if (support[i] > B) { vdjx_set_error("%s: item %zu counted in %u of %u replicates", who, i, support[i], B); return VDJX_ESTATE; }
			out_support[i] = (int32_t) support[i];
			inf.matched += support[i];
			inf.full += support[i] == B;
		}
	}
	if (info) *info = inf;
	c->stats["tree_support_batches"] = inf.batches;
	c->stats["tree_support_work_items"] = work_items;
	c->stats["tree_support_us"] = (u64) std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
	return VDJX_OK;
}
