// vdjx_lineage.hip -- clonal lineages: single linkage over the length-normalised Hamming distance of the junctions (gfx950 only, wave64).
//
//   vdjx_lineage   items of one (group, length) bucket are compared all against all; the linked pairs make a graph whose connected
//                  components are the clones (the model: include/vdjx.h; in Python: tests/lineage_model.py)
//
// The host sorts the (group, length, index) keys -- per item -- and lays the participating items out in bucket order ("rows").  Per
// pair everything happens on the device, in five dispatches whatever n and the number of buckets are:
//   k_lin_pack     a row = 8 {bases, mask} pairs in vdjx_hamming.h's format, 128 bytes (two 64-byte lines); a junction of up to 128
//                  bases lives in the first
//   k_lin_pairs    one wave per work item (row block of 64 rows, column slice of the same bucket): a lane keeps its row's live words in
//                  registers, the columns go through LDS in tiles of 64 and are read back as one 16-byte {bases, mask} broadcast per
//                  word (ham_word).  The lane keeps the smallest d > 0 (atomicMin per row at the end: the column slices of a row meet there) and,
//                  for the pairs with column > row and d <= floor(num L / den), counts the link and unites the two items
//                  (vdjx_unionfind.h, parent[] over the caller's item indices)
//   k_lin_flatten  every item's root; a flag per root, in item order
//   k_scan_one     (vdjx_scan.h) numbers the flags: the clone id of a root
//   k_lin_out      clone and nearest of every item, in the caller's order
// No floating point.  Scratch comes from the context's workspace.
//
//   vdjx_lineage_model   the same buckets, links, clones and nearest under a 5-mer substitution distance (include/vdjx.h; in Python:
//                        tests/lineage_dist_model.py).  Host layout, k_lin_pack, the union-find, k_lin_flatten, the scan and k_lin_out are
//                        the ones above; the pair pass is
//   k_lin_pairs_model    a wave per work item, the lane's row in registers and the columns through LDS tiles as in k_lin_pairs, the 8 KB
//                        table in LDS.  The host re-indexes the table to the packed rows' code order (A0 T1 C2 G3) with the 5-mer's first
//                        base in the low bits, so that the 5-mer around a position is ten adjacent bits of a row (lin_win: the two windows of
//                        a word that reach into its neighbours).  A pair first takes its Hamming count h: every counted position costs at
//                        least cmin = 2 min(1000, smallest cell), so a pair with h cmin > dmax and h cmin >= the lane's best so far can give
//                        neither a link nor a nearest and is left; the others walk the set bits of the difference mask, two look-ups each,
//                        and stop once the running sum is past both.  What is left and where a walk stops changes no result.
//   vdjx_lineage_distance_table   plain C, no GPU: the targeting weights -> the table (shazam's calcTargetingDistance in thousandths)
//   vdjx_lineage_link    the same pair pass, then complete or average linkage inside its components, cut at the threshold (include/vdjx.h;
//                        in Python: tests/lineage_link_model.py): k_link_gather, k_link_matrix / k_link_matrix_model and k_link_merge, below,
//                        between k_lin_flatten and the scan; the host's share is vdjx_link.h
#include "vdjx_common.h"
#include "vdjx_hamming.h"
#include "vdjx_link.h"
#include "vdjx_scan.h"
#include "vdjx_unionfind.h"

#include <math.h>
#include <string.h>

#define LIN_NONE 0xFFFFFFFFu
#define LIN_ROW_WORDS 8u                 // {bases, mask} pairs per row: 8 x 32 = 256 >= VDJX_LINEAGE_MAXLEN bases
#define LIN_TILE 64u                     // columns per LDS tile (the rows of a work item, HAM_ROWS, happen to be as many)

struct LinRow { u64 at; u32 item, len; };                                     // where the junction's characters start, whose they are
static_assert(sizeof(LinRow) == 16, "uploaded as it is");

// one thread per {bases, mask} pair of a row
__global__ __launch_bounds__(256) void k_lin_pack(const char* __restrict__ junc, const LinRow* __restrict__ ri, u32 rows, ulonglong2* __restrict__ out,
                                                  u32* __restrict__ row_item, u32* __restrict__ parent) {
	const u32 t = blockIdx.x * 256u + threadIdx.x, r = t / LIN_ROW_WORDS, w = t % LIN_ROW_WORDS;
	if (r >= rows) return;
	const LinRow q = ri[r];
	out[(size_t) r * LIN_ROW_WORDS + w] = ham_pack_word([&](u32 pos) { return junc[q.at + pos]; }, w, q.len);
	if (w == 0) { row_item[r] = q.item; parent[q.item] = q.item; }
}

// the register path: rows [row0, row_end) of a work item against its columns, W live words a row; u[0] of the item is the bucket's dmax
template <int W>
__device__ inline void lin_item(const HamItem it, const ulonglong2* __restrict__ rows, const u32* __restrict__ row_item, u32* parent, u32* near_,
                                unsigned long long* links, ulonglong2* tile, u32* tile_item) {
	const u32 lane = threadIdx.x, myrow = it.row0 + lane;
	const bool live = myrow < it.row_end;
	const u32 r = live ? myrow : it.row0;
	u64 x[W], m[W];
#pragma unroll
	for (int w = 0; w < W; w++) {
		const ulonglong2 q = rows[(size_t) r * LIN_ROW_WORDS + w];
		x[w] = q.x;
		m[w] = q.y;
	}
	const u32 me = row_item[r];
	u32 best = LIN_NONE, cnt = 0;
	for (u32 base = it.col0; base < it.col_end; base += LIN_TILE) {
		const u32 nc = min(LIN_TILE, it.col_end - base);
		for (u32 i = lane; i < nc * (u32) W; i += 64u) tile[i] = rows[(size_t) (base + i / (u32) W) * LIN_ROW_WORDS + i % (u32) W];
		if (lane < nc) tile_item[lane] = row_item[base + lane];
		__syncthreads();
		for (u32 c = 0; c < nc; c++) {
			u32 d = 0;
#pragma unroll
			for (int w = 0; w < W; w++) d += ham_word(x[w], m[w], tile[c * (u32) W + w]);      // (every lane the same address: one broadcast read of 16 bytes)
			const u32 p = base + c;
			if (live && p != myrow) {
				if (d != 0 && d < best) best = d;
				if (p > myrow && d <= it.u[0]) {
					cnt++;
					uf_unite(parent, me, tile_item[c]);
				}
			}
		}
		__syncthreads();
	}
	if (live && best != LIN_NONE) atomicMin(near_ + me, best);
#pragma unroll
	for (int s = 32; s >= 1; s >>= 1) cnt += (u32) __shfl_xor((int) cnt, s, 64);
	if (lane == 0 && cnt) atomicAdd(links, (unsigned long long) cnt);
}

// one wave per work item; the live words of a bucket are the same for all its rows, so the word count is uniform and every loop over
// words is unrolled (the row stays in registers)
__global__ __launch_bounds__(64) void k_lin_pairs(const HamItem* __restrict__ items, const ulonglong2* __restrict__ rows, const u32* __restrict__ row_item,
                                                  u32* parent, u32* near_, unsigned long long* links) {
	__shared__ ulonglong2 tile[LIN_TILE * LIN_ROW_WORDS];
	__shared__ u32 tile_item[LIN_TILE];
	const HamItem it = items[blockIdx.x];
	switch (it.words) {                                    // (W below is the case's constant: HAM_CASES_8 declares it)
		HAM_CASES_8(lin_item<W>(it, rows, row_item, parent, near_, links, tile, tile_item))
		default: break;
	}
}

// ---- the pair pass under the 5-mer substitution distance ------------------------------------------------------------------------------
#define LIN_TAB 4096u                    // cells of the distance table: 1,024 5-mers x 4 new bases
#define LIN_MISS 1000u                   // a side without a full ACGT 5-mer: the mean mismatch

// the two windows of a word of a stream (lo: the word before or 0, hi: the word after or 0).  near: bases -2 .. 29 of the word, base j at
// bit 2 (j + 2); far: bases 26 .. 37, base j at bit 2 (j - 26).  The 5-mer around base k of the word is ten adjacent bits of near
// (k < 28) or of far
struct LinWin { u64 near, far; };
__device__ inline LinWin lin_win(u64 lo, u64 mid, u64 hi) { return {(mid << 4) | (lo >> 60), (mid >> 52) | (hi << 12)}; }
__device__ inline u32 lin_mer(const LinWin v, u32 k) { return (u32) (k < 28u ? v.near >> (2u * k) : v.far >> (2u * (k - 28u))) & 0x3FFu; }

// rows [row0, row_end) of a work item against its columns under the table in LDS; u[0] of the item is the bucket's dmax, u[1] its length.
// counters: links, walked pairs, walked positions
template <int W>
__device__ inline void lin_item_model(const HamItem it, const ulonglong2* __restrict__ rows, const u32* __restrict__ row_item, u32* parent, u32* near_,
                                      unsigned long long* counters, ulonglong2* tile, u32* tile_item, const uint16_t* tab, u32 cmin, u32 sym) {
	const u32 lane = threadIdx.x, myrow = it.row0 + lane, dmax = it.u[0], L = it.u[1];
	const bool live = myrow < it.row_end;
	const u32 r = live ? myrow : it.row0;
	u64 x[W], m[W];
#pragma unroll
	for (int w = 0; w < W; w++) {
		const ulonglong2 q = rows[(size_t) r * LIN_ROW_WORDS + w];
		x[w] = q.x;
		m[w] = q.y;
	}
	const u32 me = row_item[r];
	u32 best = LIN_NONE, cnt = 0, walked = 0, steps = 0;
	for (u32 base = it.col0; base < it.col_end; base += LIN_TILE) {
		const u32 nc = min(LIN_TILE, it.col_end - base);
		for (u32 i = lane; i < nc * (u32) W; i += 64u) tile[i] = rows[(size_t) (base + i / (u32) W) * LIN_ROW_WORDS + i % (u32) W];
		if (lane < nc) tile_item[lane] = row_item[base + lane];
		__syncthreads();
		for (u32 c = 0; c < nc; c++) {
			ulonglong2 q[W];
			u32 h = 0;
#pragma unroll
			for (int w = 0; w < W; w++) {
				q[w] = tile[c * (u32) W + w];                                                  // (every lane the same address: one broadcast read of 16 bytes)
				h += ham_word(x[w], m[w], q[w]);
			}
			const u32 p = base + c, low = h * cmin;
			if (!live || p == myrow || (low > dmax && low >= best)) continue;                  // neither a link nor a nearer one
			walked++;
			u32 D = 0;
			bool past = false;
#pragma unroll
			for (int w = 0; w < W; w++) {
				const u64 t = x[w] ^ q[w].x;
				u64 dm = (((t | (t << 1)) & 0xAAAAAAAAAAAAAAAAull) | m[w] | q[w].y);               // bit 2k + 1: base k of the word counts
				if (past || !dm) continue;
				const LinWin xa = lin_win(w > 0 ? x[w - 1] : 0ull, x[w], w + 1 < W ? x[w + 1] : 0ull);
				const LinWin ma = lin_win(w > 0 ? m[w - 1] : 0ull, m[w], w + 1 < W ? m[w + 1] : 0ull);
				const LinWin xb = lin_win(w > 0 ? q[w - 1].x : 0ull, q[w].x, w + 1 < W ? q[w + 1].x : 0ull);
				const LinWin mb = lin_win(w > 0 ? q[w - 1].y : 0ull, q[w].y, w + 1 < W ? q[w + 1].y : 0ull);
				do {
					const u32 k = ((u32) __ffsll((unsigned long long) dm) >> 1) - 1u, pos = 32u * (u32) w + k;
					dm &= dm - 1;
					u32 ab = LIN_MISS, ba = LIN_MISS;
					if (pos >= 2u && pos + 2u < L) {
						const u32 bad_a = (u32) (m[w] >> (2u * k + 1u)) & 1u, bad_b = (u32) (q[w].y >> (2u * k + 1u)) & 1u;
						if (lin_mer(ma, k) == 0 && !bad_b) ab = tab[lin_mer(xa, k) << 2 | ((u32) (q[w].x >> (2u * k)) & 3u)];
						if (lin_mer(mb, k) == 0 && !bad_a) ba = tab[lin_mer(xb, k) << 2 | ((u32) (x[w] >> (2u * k)) & 3u)];
					}
					D += sym ? 2u * min(ab, ba) : ab + ba;
					steps++;
					past = D > dmax && D >= best;
				} while (dm && !past);
			}
			if (past) continue;
			if (D != 0 && D < best) best = D;
			if (p > myrow && D <= dmax) {
				cnt++;
				uf_unite(parent, me, tile_item[c]);
			}
		}
		__syncthreads();
	}
	if (live && best != LIN_NONE) atomicMin(near_ + me, best);
	unsigned long long all = steps;                        // (a lane's positions fit 32 bits, a wave's need not)
#pragma unroll
	for (int s = 32; s >= 1; s >>= 1) {
		cnt += (u32) __shfl_xor((int) cnt, s, 64);
		walked += (u32) __shfl_xor((int) walked, s, 64);
		all += (unsigned long long) __shfl_xor((long long) all, s, 64);
	}
	if (lane == 0 && cnt) atomicAdd(counters, (unsigned long long) cnt);
	if (lane == 0 && walked) atomicAdd(counters + 1, (unsigned long long) walked);
	if (lane == 0 && all) atomicAdd(counters + 2, all);
}

// one wave per work item, as k_lin_pairs; table: the LIN_TAB cells in the rows' code order
__global__ __launch_bounds__(64) void k_lin_pairs_model(const HamItem* __restrict__ items, const ulonglong2* __restrict__ rows, const u32* __restrict__ row_item,
                                                        u32* parent, u32* near_, unsigned long long* counters, const uint4* __restrict__ table, u32 cmin, u32 sym) {
	__shared__ ulonglong2 tile[LIN_TILE * LIN_ROW_WORDS];
	__shared__ u32 tile_item[LIN_TILE];
	__shared__ uint4 tab[LIN_TAB / 8u];
	for (u32 i = threadIdx.x; i < LIN_TAB / 8u; i += 64u) tab[i] = table[i];
	__syncthreads();
	const HamItem it = items[blockIdx.x];
	switch (it.words) {                                    // (W below is the case's constant: HAM_CASES_8 declares it)
		HAM_CASES_8(lin_item_model<W>(it, rows, row_item, parent, near_, counters, tile, tile_item, (const uint16_t*) tab, cmin, sym))
		default: break;
	}
}

__global__ __launch_bounds__(256) void k_lin_flatten(const u32* __restrict__ parent, u32 n, u32* __restrict__ root, u32* __restrict__ flag) {
	const u32 i = blockIdx.x * 256u + threadIdx.x;
	if (i >= n) return;
	u32 r = parent[i];
	if (r != LIN_NONE)
		for (u32 p = parent[r]; p != r; p = parent[r]) r = p;
	root[i] = r;
	flag[i] = r == i ? 1u : 0u;
}

__global__ __launch_bounds__(256) void k_lin_out(const u32* __restrict__ root, const u32* __restrict__ number, const u32* __restrict__ near_, u32 n,
                                                 int32_t* __restrict__ out_clone, int32_t* __restrict__ out_nearest) {
	const u32 i = blockIdx.x * 256u + threadIdx.x;
	if (i >= n) return;
	const u32 r = root[i], d = near_[i];
	out_clone[i] = r == LIN_NONE ? -1 : (int32_t) number[r];
	out_nearest[i] = r == LIN_NONE || d == LIN_NONE ? -1 : (int32_t) d;
}

// ---- complete and average linkage (vdjx_lineage_link) ----------------------------------------------------------------------------------
// Only the single-linkage components of the pair pass are agglomerated (include/vdjx.h says why no merge crosses two of them).  The host
// puts the rows of the components of two and more in component order (vdjx_link.h) and cuts them into batches; per batch
//   k_link_matrix / k_link_matrix_model   the full m x m matrix of every component, as work items (component, row block, column slice):
//                  u[0] the matrix's first cell, u[1] = L | m << 8, u[2] the component's first row.  The loops are lin_item's and
//                  lin_item_model's, kept apart from them (profiles/hamming_engine_refactor_check.md), without the filter and the early
//                  exit: a cell holds the true D.  D is symmetric, so the lane of row r writes cell [column][r] and a wave's stores of one
//                  column are adjacent
//   k_link_merge   one workgroup per component: the agglomeration under the strict order (delta, id(A), id(B)), local index for id
// A cell is 4 bytes under complete linkage (a maximum of D's) and 8 under average (a sum of them, below 2^41).
#define LINK_LDS_M 88u                   // components up to here keep matrix and state in LDS: 88 * 88 * 8 + 88 * 20 = 63,712 bytes, two workgroups a CU
#define LINK_THREADS 256u
#define LINK_WAVES (LINK_THREADS / 64u)

struct LinkComp { u32 first, m, base, L; u64 K; };                            // rows [first, first + m) of the component order, cells from base, K = unit num L
struct LinkState { u64 S; u32 j, size; };                                     // per cluster: its row's smallest eligible key (S, partner j > itself; LIN_NONE: none), size (0: merged into j)
static_assert(sizeof(LinkComp) == 24 && sizeof(LinkState) == 16, "uploaded as it is");

// one thread per {bases, mask} pair of a row of the component order
__global__ __launch_bounds__(256) void k_link_gather(const ulonglong2* __restrict__ rows, const u32* __restrict__ row_item, const u32* __restrict__ perm, u32 n_rows,
                                                     ulonglong2* __restrict__ out, u32* __restrict__ out_item) {
	const u32 t = blockIdx.x * 256u + threadIdx.x, r = t / LIN_ROW_WORDS, w = t % LIN_ROW_WORDS;
	if (r >= n_rows) return;
	const u32 from = perm[r];
	out[(size_t) r * LIN_ROW_WORDS + w] = rows[(size_t) from * LIN_ROW_WORDS + w];
	if (w == 0) out_item[r] = row_item[from];
}

__device__ inline void link_store(void* mat, u32 wide, size_t cell, u32 d) {
	if (wide) ((u64*) mat)[cell] = d;
	else ((u32*) mat)[cell] = d;
}

template <int W>
__device__ inline void link_item(const HamItem it, const ulonglong2* __restrict__ rows, void* mat, u32 wide, ulonglong2* tile) {
	const u32 lane = threadIdx.x, myrow = it.row0 + lane, m = it.u[1] >> 8, first = it.u[2];
	const bool live = myrow < it.row_end;
	const u32 r = live ? myrow : it.row0;
	u64 x[W], mk[W];
#pragma unroll
	for (int w = 0; w < W; w++) {
		const ulonglong2 q = rows[(size_t) r * LIN_ROW_WORDS + w];
		x[w] = q.x;
		mk[w] = q.y;
	}
	for (u32 base = it.col0; base < it.col_end; base += LIN_TILE) {
		const u32 nc = min(LIN_TILE, it.col_end - base);
		for (u32 i = lane; i < nc * (u32) W; i += 64u) tile[i] = rows[(size_t) (base + i / (u32) W) * LIN_ROW_WORDS + i % (u32) W];
		__syncthreads();
		for (u32 c = 0; c < nc; c++) {
			u32 d = 0;
#pragma unroll
			for (int w = 0; w < W; w++) d += ham_word(x[w], mk[w], tile[c * (u32) W + w]);
			if (live) link_store(mat, wide, (size_t) it.u[0] + (size_t) (base + c - first) * m + (myrow - first), d);
		}
		__syncthreads();
	}
}

__global__ __launch_bounds__(64) void k_link_matrix(const HamItem* __restrict__ items, const ulonglong2* __restrict__ rows, void* mat, u32 wide) {
	__shared__ ulonglong2 tile[LIN_TILE * LIN_ROW_WORDS];
	const HamItem it = items[blockIdx.x];
	switch (it.words) {                                    // (W below is the case's constant: HAM_CASES_8 declares it)
		HAM_CASES_8(link_item<W>(it, rows, mat, wide, tile))
		default: break;
	}
}

template <int W>
__device__ inline void link_item_model(const HamItem it, const ulonglong2* __restrict__ rows, void* mat, u32 wide, ulonglong2* tile, const uint16_t* tab, u32 sym) {
	const u32 lane = threadIdx.x, myrow = it.row0 + lane, L = it.u[1] & 0xFFu, m = it.u[1] >> 8, first = it.u[2];
	const bool live = myrow < it.row_end;
	const u32 r = live ? myrow : it.row0;
	u64 x[W], mk[W];
#pragma unroll
	for (int w = 0; w < W; w++) {
		const ulonglong2 q = rows[(size_t) r * LIN_ROW_WORDS + w];
		x[w] = q.x;
		mk[w] = q.y;
	}
	for (u32 base = it.col0; base < it.col_end; base += LIN_TILE) {
		const u32 nc = min(LIN_TILE, it.col_end - base);
		for (u32 i = lane; i < nc * (u32) W; i += 64u) tile[i] = rows[(size_t) (base + i / (u32) W) * LIN_ROW_WORDS + i % (u32) W];
		__syncthreads();
		for (u32 c = 0; c < nc; c++) {
			ulonglong2 q[W];
#pragma unroll
			for (int w = 0; w < W; w++) q[w] = tile[c * (u32) W + w];
			u32 D = 0;
#pragma unroll
			for (int w = 0; w < W; w++) {
				const u64 t = x[w] ^ q[w].x;
				u64 dm = (((t | (t << 1)) & 0xAAAAAAAAAAAAAAAAull) | mk[w] | q[w].y);              // bit 2k + 1: base k of the word counts
				if (!dm) continue;
				const LinWin xa = lin_win(w > 0 ? x[w - 1] : 0ull, x[w], w + 1 < W ? x[w + 1] : 0ull);
				const LinWin ma = lin_win(w > 0 ? mk[w - 1] : 0ull, mk[w], w + 1 < W ? mk[w + 1] : 0ull);
				const LinWin xb = lin_win(w > 0 ? q[w - 1].x : 0ull, q[w].x, w + 1 < W ? q[w + 1].x : 0ull);
				const LinWin mb = lin_win(w > 0 ? q[w - 1].y : 0ull, q[w].y, w + 1 < W ? q[w + 1].y : 0ull);
				do {
					const u32 k = ((u32) __ffsll((unsigned long long) dm) >> 1) - 1u, pos = 32u * (u32) w + k;
					dm &= dm - 1;
					u32 ab = LIN_MISS, ba = LIN_MISS;
					if (pos >= 2u && pos + 2u < L) {
						const u32 bad_a = (u32) (mk[w] >> (2u * k + 1u)) & 1u, bad_b = (u32) (q[w].y >> (2u * k + 1u)) & 1u;
						if (lin_mer(ma, k) == 0 && !bad_b) ab = tab[lin_mer(xa, k) << 2 | ((u32) (q[w].x >> (2u * k)) & 3u)];
						if (lin_mer(mb, k) == 0 && !bad_a) ba = tab[lin_mer(xb, k) << 2 | ((u32) (x[w] >> (2u * k)) & 3u)];
					}
					D += sym ? 2u * min(ab, ba) : ab + ba;
				} while (dm);
			}
			if (live) link_store(mat, wide, (size_t) it.u[0] + (size_t) (base + c - first) * m + (myrow - first), D);
		}
		__syncthreads();
	}
}

__global__ __launch_bounds__(64) void k_link_matrix_model(const HamItem* __restrict__ items, const ulonglong2* __restrict__ rows, void* mat, u32 wide,
                                                          const uint4* __restrict__ table, u32 sym) {
	__shared__ ulonglong2 tile[LIN_TILE * LIN_ROW_WORDS];
	__shared__ uint4 tab[LIN_TAB / 8u];
	for (u32 i = threadIdx.x; i < LIN_TAB / 8u; i += 64u) tab[i] = table[i];
	__syncthreads();
	const HamItem it = items[blockIdx.x];
	switch (it.words) {                                    // (W below is the case's constant: HAM_CASES_8 declares it)
		HAM_CASES_8(link_item_model<W>(it, rows, mat, wide, tile, (const uint16_t*) tab, sym))
		default: break;
	}
}

// a candidate pair: S over n (n: |A| |B| under average linkage, 1 under complete), the two local indices; j == LIN_NONE: none
struct LinkKey { u64 S, n; u32 i, j; };

// the strict order (delta, id(A), id(B)), delta compared exactly: only eligible pairs get here, S n < 2^63 (include/vdjx.h)
__device__ inline bool link_less(const LinkKey a, const LinkKey b) {
	if (a.j == LIN_NONE || b.j == LIN_NONE) return b.j == LIN_NONE && a.j != LIN_NONE;
	const u64 l = a.S * b.n, r = b.S * a.n;
	if (l != r) return l < r;
	return a.i != b.i ? a.i < b.i : a.j < b.j;
}

__device__ inline LinkKey link_wave_min(LinkKey k) {
#pragma unroll
	for (int s = 32; s >= 1; s >>= 1) {
		LinkKey o;
		o.S = (u64) __shfl_xor((long long) k.S, s, 64);
		o.n = (u64) __shfl_xor((long long) k.n, s, 64);
		o.i = (u32) __shfl_xor((int) k.i, s, 64);
		o.j = (u32) __shfl_xor((int) k.j, s, 64);
		if (link_less(o, k)) k = o;
	}
	return k;
}

// Cell = u32: complete linkage, u64: average.  mat, state and list are the batch's (cells from comps[].base, entries from comps[].first)
// and used by the components above LINK_LDS_M; the others copy their matrix into LDS.  item: the rows' items in component order; root and
// flag get every member's final cluster (its smallest member) and whether it is that member
template <typename Cell>
__global__ __launch_bounds__(LINK_THREADS) void k_link_merge(const LinkComp* __restrict__ comps, Cell* mat, LinkState* state, u32* list, const u32* __restrict__ item,
                                                             u32 den, u32* __restrict__ root, u32* __restrict__ flag) {
	constexpr bool AVG = sizeof(Cell) == 8;
	__shared__ Cell l_mat[LINK_LDS_M * LINK_LDS_M];
	__shared__ LinkState l_state[LINK_LDS_M];
	__shared__ u32 l_list[LINK_LDS_M];
	__shared__ LinkKey red[LINK_WAVES];
	__shared__ u32 n_list;
	const LinkComp cp = comps[blockIdx.x];
	const u32 m = cp.m, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
	const u64 kd = cp.K / den;                             // complete: eligible iff S <= floor(K / den)
	Cell* M = mat + cp.base;
	LinkState* st = state + cp.first;
	u32* lst = list + cp.first;
	if (m <= LINK_LDS_M) {
		for (u32 i = tid; i < m * m; i += LINK_THREADS) l_mat[i] = M[i];
		M = l_mat;
		st = l_state;
		lst = l_list;
	}
	for (u32 c = tid; c < m; c += LINK_THREADS) st[c] = {0ull, LIN_NONE, 1u};
	__syncthreads();

	// the smallest eligible key of row c among the live j > c, by one wave
	auto scan_row = [&](u32 c) {
		const u64 nc = st[c].size;
		LinkKey best = {0ull, 1ull, c, LIN_NONE};
		for (u32 j = c + 1u + lane; j < m; j += 64u) {
			const u64 nj = st[j].size;
			if (!nj) continue;
			const LinkKey k = {(u64) M[(size_t) c * m + j], AVG ? nc * nj : 1ull, c, j};
			if (k.S <= (AVG ? cp.K * k.n / den : kd) && link_less(k, best)) best = k;
		}
		best = link_wave_min(best);
		if (lane == 0) { st[c].S = best.S; st[c].j = best.j; }
	};
	for (u32 c = wave; c + 1u < m; c += LINK_WAVES) scan_row(c);
	__syncthreads();

	for (;;) {
		LinkKey best = {0ull, 1ull, 0u, LIN_NONE};
		for (u32 c = tid; c < m; c += LINK_THREADS) {
			const LinkState s = st[c];
			if (!s.size || s.j == LIN_NONE) continue;
			const LinkKey k = {s.S, AVG ? (u64) s.size * st[s.j].size : 1ull, c, s.j};
			if (link_less(k, best)) best = k;
		}
		best = link_wave_min(best);
		if (lane == 0) red[wave] = best;
		if (tid == 0) n_list = 0;
		__syncthreads();
		best = red[0];
#pragma unroll
		for (u32 w = 1; w < LINK_WAVES; w++)
			if (link_less(red[w], best)) best = red[w];
		if (best.j == LIN_NONE) break;                     // (every thread sees the same four keys)
		const u32 a = best.i, b = best.j;
		for (u32 c = tid; c < m; c += LINK_THREADS) {       // Lance-Williams, exact: max, or the sum of the sums
			if (c == a || c == b || !st[c].size) continue;
			const Cell va = M[(size_t) a * m + c], vb = M[(size_t) b * m + c], v = AVG ? va + vb : (va > vb ? va : vb);
			M[(size_t) a * m + c] = v;
			M[(size_t) c * m + a] = v;
		}
		__syncthreads();
		if (tid == 0) {
			st[a].size += st[b].size;
			st[b].size = 0;
			st[b].j = a;
		}
		__syncthreads();
		// the caches: A's own row and the rows that pointed at A or B are scanned again, a row before A takes its new pair with A if that
		// is smaller; every other row's cached pair is untouched by the merge
		const u64 na = st[a].size;
		for (u32 c = tid; c < b; c += LINK_THREADS) {
			const LinkState s = st[c];
			if (!s.size) continue;
			if (c == a || s.j == a || s.j == b) lst[atomicAdd(&n_list, 1u)] = c;          // (the order of the list shows nowhere: a row's scan is its own)
			else if (c < a) {
				const LinkKey k = {(u64) M[(size_t) c * m + a], AVG ? (u64) s.size * na : 1ull, c, a};
				const LinkKey old = {s.S, s.j == LIN_NONE ? 1ull : AVG ? (u64) s.size * st[s.j].size : 1ull, c, s.j};
				if (k.S <= (AVG ? cp.K * k.n / den : kd) && link_less(k, old)) { st[c].S = k.S; st[c].j = a; }
			}
		}
		__syncthreads();
		const u32 nl = n_list;
		for (u32 k = wave; k < nl; k += LINK_WAVES) scan_row(lst[k]);
		__syncthreads();
	}
	for (u32 c = tid; c < m; c += LINK_THREADS) {
		u32 r = c;
		while (!st[r].size) r = st[r].j;
		const u32 me = item[cp.first + c];
		root[me] = item[cp.first + r];
		flag[me] = r == c ? 1u : 0u;
	}
}

// the cells of a distance table in the rows' code order: index (v << 2 | y), v the ten bits of a 5-mer as they lie in a packed row (its first
// base lowest), y the new base, both in vdjx_hamming.h's codes (A0 T1 C2 G3); the caller's table is row 256 a + 64 b + 16 c + 4 d + e, column
// the new base, in A0 C1 G2 T3
static void lin_table_reindex(const uint16_t* table, uint16_t* out) {
	static const u32 std_of[4] = {0u, 3u, 1u, 2u};         // A T C G -> A0 C1 G2 T3
	for (u32 v = 0; v < 1024u; v++) {
		u32 idx = 0;
		for (u32 j = 0; j < 5u; j++) idx = 4u * idx + std_of[(v >> (2u * j)) & 3u];
		for (u32 y = 0; y < 4u; y++) out[v << 2 | y] = table[4u * idx + std_of[y]];
	}
}

// complete (1) or average (2) linkage over the components of the finished pair pass.  d_root: every item's root, from k_lin_flatten; it and
// d_flag come back with the final clusters of the members of every component of two and more.  The stream is waited for once, for the roots
static int link_run(const char* fn, vdjx_ctx* c, vdjx_work& wk, const std::vector<LinRow>& ri, u32 n, int num, int den, u32 unit, const uint4* d_table, u32 sym,
                    int linkage, const ulonglong2* d_rows, const u32* d_row_item, u32* d_root, u32* d_flag, vdjx_lineage_link_info* lk) {
	hipStream_t st = c->stream;
	std::vector<u32> root(n);
	HIP_TRY(hipMemcpyAsync(root.data(), d_root, n * sizeof(u32), hipMemcpyDeviceToHost, st));
	HIP_TRY(hipStreamSynchronize(st));
	LinkOrder o;
	if (!link_order(root.data(), n, o)) { vdjx_set_error("%s: the pair pass left a root that is none", fn); return VDJX_EHIP; }
	lk->components = (u32) o.size.size();
	lk->largest_component = o.largest;
	lk->clones_single = o.clones_single;
	if (o.largest > LINK_MAX_M) {
		vdjx_set_error("%s: a single-linkage component of %u junctions (at most %u under complete or average linkage)", fn, o.largest, LINK_MAX_M);
		return VDJX_ELIMIT;
	}
	if (o.size.empty()) return VDJX_OK;
	const u64 knob = (u64) vdjx_env_num("VDJX_LINK_CELLS", 1ll << 26, 1, 1ll << 28);
	std::vector<u32> end;
	link_batches(o.size, knob, end);
	const u32 total = (u32) o.member.size(), wide = linkage == 2 ? 1u : 0u;
	std::vector<u32> row_of(n, LIN_NONE), perm(total);
	for (u32 r = 0; r < (u32) ri.size(); r++) row_of[ri[r].item] = r;
	for (u32 p = 0; p < total; p++) perm[p] = row_of[o.member[p]];
	std::vector<LinkComp> comps(o.size.size());
	std::vector<HamItem> items;
	std::vector<size_t> item_end;                          // per batch: one past its last work item
	u64 most = 0;
	for (size_t b = 0, k = 0; b < end.size(); b++) {
		u64 cells = 0;
		for (size_t q = k; q < end[b]; q++) cells += (u64) o.size[q] * o.size[q];
		const u32 slice = ham_slice_width(cells);
		u64 base = 0;                                      // (a batch is at most 2^28 cells: the knob's range, or one component of 4,096)
		for (; k < end[b]; k++) {
			const u32 m = o.size[k], L = ri[perm[o.first[k]]].len;
			comps[k] = {o.first[k], m, (u32) base, L, (u64) unit * (u64) num * L};
			ham_slice_items({o.first[k], m, (L + 31u) / 32u, {(u32) base, L | m << 8, o.first[k]}}, slice, items);
			base += (u64) m * m;
		}
		item_end.push_back(items.size());
		most = std::max(most, cells);
		lk->cells += cells;
	}
	lk->batches = (u32) end.size();

	u32 *d_perm, *d_item, *d_list;
	ulonglong2* d_crows;
	LinkComp* d_comps;
	HamItem* d_items;
	LinkState* d_state;
	u64* d_mat;
	HIP_TRY(wk.alloc(&d_perm, total));
	HIP_TRY(wk.alloc(&d_item, total));
	HIP_TRY(wk.alloc(&d_list, total));
	HIP_TRY(wk.alloc(&d_crows, (size_t) total * LIN_ROW_WORDS));
	HIP_TRY(wk.alloc(&d_comps, comps.size()));
	HIP_TRY(wk.alloc(&d_items, items.size()));
	HIP_TRY(wk.alloc(&d_state, total));
	HIP_TRY(wk.alloc(&d_mat, wide ? (size_t) most : (size_t) ((most + 1) / 2)));
	HIP_TRY(hipMemcpyAsync(d_perm, perm.data(), total * sizeof(u32), hipMemcpyHostToDevice, st));
	HIP_TRY(hipMemcpyAsync(d_comps, comps.data(), comps.size() * sizeof(LinkComp), hipMemcpyHostToDevice, st));
	HIP_TRY(hipMemcpyAsync(d_items, items.data(), items.size() * sizeof(HamItem), hipMemcpyHostToDevice, st));
	{
		vdjx_prof_scope ps(c, "k_link_gather");
		hipLaunchKernelGGL(k_link_gather, dim3((total * LIN_ROW_WORDS + 255u) / 256u), dim3(256), 0, st, d_rows, d_row_item, (const u32*) d_perm, total, d_crows, d_item);
	}
	for (size_t b = 0; b < end.size(); b++) {
		const size_t i0 = b ? item_end[b - 1] : 0, k0 = b ? end[b - 1] : 0;
		const u32 ni = (u32) (item_end[b] - i0), nk = (u32) (end[b] - k0);
		{
			vdjx_prof_scope ps(c, "k_link_matrix");
			if (!d_table)
				hipLaunchKernelGGL(k_link_matrix, dim3(ni), dim3(64), 0, st, (const HamItem*) d_items + i0, (const ulonglong2*) d_crows, (void*) d_mat, wide);
			else
				hipLaunchKernelGGL(k_link_matrix_model, dim3(ni), dim3(64), 0, st, (const HamItem*) d_items + i0, (const ulonglong2*) d_crows, (void*) d_mat, wide, d_table, sym);
		}
		{
			vdjx_prof_scope ps(c, "k_link_merge");
			if (wide)
				hipLaunchKernelGGL(k_link_merge<u64>, dim3(nk), dim3(LINK_THREADS), 0, st, (const LinkComp*) d_comps + k0, d_mat, d_state, d_list, (const u32*) d_item,
				                   (u32) den, d_root, d_flag);
			else
				hipLaunchKernelGGL(k_link_merge<u32>, dim3(nk), dim3(LINK_THREADS), 0, st, (const LinkComp*) d_comps + k0, (u32*) d_mat, d_state, d_list, (const u32*) d_item,
				                   (u32) den, d_root, d_flag);
		}
	}
	return VDJX_OK;
}

// what vdjx_lineage and vdjx_lineage_model share: the checks, the host layout and every dispatch but the pair pass.  table == NULL: the
// Hamming pass; otherwise the caller's checked table, dmax in units of 2000 a position.  linkage 1, 2 (vdjx_lineage_link): the components
// of the pair pass are agglomerated before they are numbered; 0 launches what it always did
static int lin_run(const char* fn, vdjx_ctx* c, const char* junctions, const uint64_t* off, const uint32_t* group, size_t n, int num, int den,
                   const uint16_t* table, u32 sym, int32_t* out_clone, int32_t* out_nearest, vdjx_lineage_info* info, int linkage = 0,
                   vdjx_lineage_link_info* link = nullptr) {
	if (den < 1 || den > 1000000 || num < 0 || num > den) {
		vdjx_set_error("%s: threshold %d/%d (den 1 .. 10^6, num 0 .. den)", fn, num, den);
		return VDJX_EINVAL;
	}
	if (n == 0) return VDJX_OK;
	if (!junctions || !off || !group || !out_clone) { vdjx_set_error("%s: NULL argument", fn); return VDJX_EINVAL; }
	if (n >= (1ull << 20)) { vdjx_set_error("%s: %zu items (at most 2^20 - 1 per call)", fn, n); return VDJX_EINVAL; }
	const auto t0 = std::chrono::steady_clock::now();
	std::vector<u64> keys;                                 // group << 28 | length << 20 | index: the bucket order
	for (size_t i = 0; i < n; i++) {
		if (off[i + 1] < off[i]) { vdjx_set_error("%s: offsets of item %zu decrease", fn, i); return VDJX_EINVAL; }
		if (group[i] == VDJX_LINEAGE_NONE) continue;
		const u64 L = off[i + 1] - off[i];
		if (L == 0 || L > VDJX_LINEAGE_MAXLEN) {
			vdjx_set_error("%s: item %zu has %llu bases (1 .. %d)", fn, i, (unsigned long long) L, VDJX_LINEAGE_MAXLEN);
			return VDJX_EINVAL;
		}
		keys.push_back((u64) group[i] << 28 | L << 20 | (u64) i);
	}
	const u32 rows = (u32) keys.size();
	vdjx_lineage_info inf;
	memset(&inf, 0, sizeof inf);
	inf.items = rows;
	if (rows == 0) {
		for (size_t i = 0; i < n; i++) { out_clone[i] = -1; if (out_nearest) out_nearest[i] = -1; }
		if (info) *info = inf;
		c->stats["lineage_work_items"] = 0;
		c->stats["lineage_us"] = 0;
		if (table) c->stats["lineage_model_walked"] = c->stats["lineage_model_positions"] = 0;
		if (linkage) c->stats["lineage_link_us"] = c->stats["lineage_link_cells"] = 0;
		return VDJX_OK;
	}
	std::sort(keys.begin(), keys.end());
	std::vector<LinRow> ri(rows);
	std::vector<uint2> buckets;                            // first row, rows
	u64 cells = 0;
	for (u32 r = 0; r < rows; r++) {
		const u32 i = (u32) (keys[r] & 0xFFFFFu);
		ri[r] = {off[i] - off[0], i, (u32) (off[i + 1] - off[i])};
		if (r == 0 || (keys[r] >> 20) != (keys[r - 1] >> 20)) buckets.push_back(make_uint2(r, 0));
		buckets.back().y++;
	}
	for (const uint2& b : buckets) {
		inf.largest_bucket = std::max(inf.largest_bucket, b.y);
		inf.pairs += (u64) b.y * (b.y - 1) / 2;
		cells += (u64) b.y * b.y;
	}
	inf.buckets = (u32) buckets.size();
	const u32 slice = ham_slice_width(cells);
	std::vector<HamItem> items;                            // a bucket is a group; its user word: dmax
	for (const uint2& b : buckets) {
		const u32 L = ri[b.x].len;
		// d * den <= num * L  <=>  d <= floor(num * L / den); under a table D * den <= 2000 * num * L (at most 510,000)
		const u32 dmax = (u32) ((table ? 2000ull : 1ull) * (u64) num * L / (u64) den);
		ham_slice_items({b.x, b.y, (L + 31u) / 32u, {dmax, L, 0u}}, slice, items);
	}
	std::vector<uint16_t> packed;                          // the table as the device reads it, and the least a counted position costs
	u32 cmin = 2u * LIN_MISS;
	if (table) {
		packed.resize(LIN_TAB);
		lin_table_reindex(table, packed.data());
		for (u32 i = 0; i < LIN_TAB; i++)
			if (((i >> 6) & 3u) != (i & 3u)) cmin = std::min(cmin, 2u * (u32) table[i]);
#ifdef VDJX_ABLATE                  // profiles/lineage_model_at_size.py: the pair pass without its pre-filter (a bound of 0 leaves no pair)
		if (vdjx_env_set("VDJX_LIN_NOFILTER")) cmin = 0;
#endif
	}

	HIP_TRY(hipSetDevice(c->device));
	hipStream_t st = c->stream;
	vdjx_work wk(c);
	const size_t jbytes = (size_t) (off[n] - off[0]);
	char* d_junc;
	LinRow* d_ri;
	HamItem* d_items;
	ulonglong2* d_rows;
	u32 *d_row_item, *d_state, *d_root, *d_flag, *d_number;
	unsigned long long* d_links;                           // links, walked pairs, walked positions
	uint16_t* d_table = nullptr;
	int32_t* d_out;
	HIP_TRY(wk.alloc(&d_junc, jbytes));
	HIP_TRY(wk.alloc(&d_ri, rows));
	HIP_TRY(wk.alloc(&d_items, items.size()));
	HIP_TRY(wk.alloc(&d_rows, (size_t) rows * LIN_ROW_WORDS));
	HIP_TRY(wk.alloc(&d_row_item, rows));
	HIP_TRY(wk.alloc(&d_state, 2 * n));                   // parent | nearest, both all ones to begin with
	HIP_TRY(wk.alloc(&d_root, n));
	HIP_TRY(wk.alloc(&d_flag, n));
	HIP_TRY(wk.alloc(&d_number, n + 1));
	HIP_TRY(wk.alloc(&d_links, 3));
	if (table) HIP_TRY(wk.alloc(&d_table, LIN_TAB));
	HIP_TRY(wk.alloc(&d_out, 2 * n));
	u32 *d_parent = d_state, *d_near = d_state + n;
	if (jbytes) HIP_TRY(hipMemcpyAsync(d_junc, junctions + off[0], jbytes, hipMemcpyHostToDevice, st));
	HIP_TRY(hipMemcpyAsync(d_ri, ri.data(), rows * sizeof(LinRow), hipMemcpyHostToDevice, st));
	HIP_TRY(hipMemcpyAsync(d_items, items.data(), items.size() * sizeof(HamItem), hipMemcpyHostToDevice, st));
	HIP_TRY(hipMemsetAsync(d_state, 0xFF, 2 * n * sizeof(u32), st));
	if (table) HIP_TRY(hipMemcpyAsync(d_table, packed.data(), LIN_TAB * sizeof(uint16_t), hipMemcpyHostToDevice, st));
	HIP_TRY(hipMemsetAsync(d_links, 0, 3 * sizeof(unsigned long long), st));
	const u32 nb = (u32) ((n + 255) / 256);
	{
		vdjx_prof_scope ps(c, "k_lin_pack");
		hipLaunchKernelGGL(k_lin_pack, dim3((rows * LIN_ROW_WORDS + 255u) / 256u), dim3(256), 0, st, (const char*) d_junc, (const LinRow*) d_ri, rows, d_rows,
		                   d_row_item, d_parent);
	}
	if (!table) {
		vdjx_prof_scope ps(c, "k_lin_pairs");
		hipLaunchKernelGGL(k_lin_pairs, dim3((u32) items.size()), dim3(64), 0, st, (const HamItem*) d_items, (const ulonglong2*) d_rows,
		                   (const u32*) d_row_item, d_parent, d_near, d_links);
	} else {
		vdjx_prof_scope ps(c, "k_lin_pairs_model");
		hipLaunchKernelGGL(k_lin_pairs_model, dim3((u32) items.size()), dim3(64), 0, st, (const HamItem*) d_items, (const ulonglong2*) d_rows,
		                   (const u32*) d_row_item, d_parent, d_near, d_links, (const uint4*) d_table, cmin, sym);
	}
	{
		vdjx_prof_scope ps(c, "k_lin_flatten");
		hipLaunchKernelGGL(k_lin_flatten, dim3(nb), dim3(256), 0, st, (const u32*) d_parent, (u32) n, d_root, d_flag);
	}
	vdjx_lineage_link_info lk;
	memset(&lk, 0, sizeof lk);
	if (linkage) {
		const auto t1 = std::chrono::steady_clock::now();
		const int rc = link_run(fn, c, wk, ri, (u32) n, num, den, table ? 2000u : 1u, (const uint4*) d_table, sym, linkage, (const ulonglong2*) d_rows,
		                        (const u32*) d_row_item, d_root, d_flag, &lk);
		if (rc) return rc;
		c->stats["lineage_link_us"] = (u64) std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t1).count();
		c->stats["lineage_link_cells"] = lk.cells;
	}
	{
		vdjx_prof_scope ps(c, "k_lin_number");
		vdjx_scan_one(st, (const u32*) d_flag, (u32) n, d_number);
	}
	{
		vdjx_prof_scope ps(c, "k_lin_out");
		hipLaunchKernelGGL(k_lin_out, dim3(nb), dim3(256), 0, st, (const u32*) d_root, (const u32*) d_number, (const u32*) d_near, (u32) n, d_out, d_out + n);
	}
	unsigned long long links[3] = {0, 0, 0};
	u32 clones = 0;
	HIP_TRY(hipMemcpyAsync(out_clone, d_out, n * sizeof(int32_t), hipMemcpyDeviceToHost, st));
	if (out_nearest) HIP_TRY(hipMemcpyAsync(out_nearest, d_out + n, n * sizeof(int32_t), hipMemcpyDeviceToHost, st));
	HIP_TRY(hipMemcpyAsync(links, d_links, sizeof links, hipMemcpyDeviceToHost, st));
	HIP_TRY(hipMemcpyAsync(&clones, d_number + n, sizeof clones, hipMemcpyDeviceToHost, st));
	HIP_TRY(hipStreamSynchronize(st));
	HIP_TRY(hipGetLastError());
	vdjx_prof_collect(c, false);
	inf.links = links[0];
	inf.clones = clones;
	if (info) *info = inf;
	lk.merges = linkage ? rows - clones : 0u;              // (every merge makes one cluster of two, and the rows begin as clusters)
	if (link) *link = lk;
	c->stats["lineage_work_items"] = items.size();
	c->stats["lineage_us"] = (u64) std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
	if (table) {
		c->stats["lineage_model_walked"] = links[1];
		c->stats["lineage_model_positions"] = links[2];
	}
	return VDJX_OK;
}

extern "C" int vdjx_lineage(vdjx_ctx* c, const char* junctions, const uint64_t* off, const uint32_t* group, size_t n, const vdjx_lineage_params* prm,
                            int32_t* out_clone, int32_t* out_nearest, vdjx_lineage_info* info) {
	if (info) memset(info, 0, sizeof *info);
	if (!c || !prm) { vdjx_set_error("vdjx_lineage: NULL argument"); return VDJX_EINVAL; }
	return lin_run("vdjx_lineage", c, junctions, off, group, n, prm->num, prm->den, nullptr, 0u, out_clone, out_nearest, info);
}

extern "C" int vdjx_lineage_model(vdjx_ctx* c, const char* junctions, const uint64_t* off, const uint32_t* group, size_t n, const vdjx_lineage_model_params* prm,
                                  const uint16_t* table, int32_t* out_clone, int32_t* out_nearest, vdjx_lineage_info* info) {
	if (info) memset(info, 0, sizeof *info);
	if (!c || !prm) { vdjx_set_error("vdjx_lineage_model: NULL argument"); return VDJX_EINVAL; }
	if (prm->symmetry != 0 && prm->symmetry != 1) { vdjx_set_error("vdjx_lineage_model: symmetry %d (0: avg, 1: min)", prm->symmetry); return VDJX_EINVAL; }
	if (!table) { vdjx_set_error("vdjx_lineage_model: NULL table"); return VDJX_EINVAL; }
	for (u32 i = 0; i < LIN_TAB; i++)
		if (((i >> 6) & 3u) != (i & 3u) && table[i] == 0) {
			vdjx_set_error("vdjx_lineage_model: the table's cell [%u][%u] is 0 (an off-centre cell is 1 .. 65535)", i >> 2, i & 3u);
			return VDJX_EINVAL;
		}
	return lin_run("vdjx_lineage_model", c, junctions, off, group, n, prm->num, prm->den, table, (u32) prm->symmetry, out_clone, out_nearest, info);
}

// plain C, no GPU: -log10 of the targeting probability, normalised to a mean of 1, in thousandths.  One float64 operation per statement and
// the sum in index order: the Python model (tests/lineage_dist_model.py), which calls the same libm in the same order, gives the same integers
extern "C" int vdjx_lineage_distance_table(const uint32_t* weight, uint16_t* table, vdjx_lineage_table_info* info) {
	if (info) memset(info, 0, sizeof *info);
	if (!weight || !table) { vdjx_set_error("vdjx_lineage_distance_table: NULL argument"); return VDJX_EINVAL; }
	u64 S = 0;
	for (u32 i = 0; i < LIN_TAB; i++)
		if (((i >> 6) & 3u) != (i & 3u)) S += std::max(weight[i], 1u);
	std::vector<double> d(LIN_TAB, 0.0);
	double sum = 0.0;
	for (u32 i = 0; i < LIN_TAB; i++) {
		if (((i >> 6) & 3u) == (i & 3u)) continue;
		const double ratio = (double) std::max(weight[i], 1u) / (double) S;
		d[i] = -log10(ratio);
		sum += d[i];
	}
	const double mean = sum / 3072.0;
	u32 lo = 65535u, hi = 1u;
	for (u32 i = 0; i < LIN_TAB; i++) {
		if (((i >> 6) & 3u) == (i & 3u)) { table[i] = 0; continue; }
		const double scaled = 1000.0 * d[i];
		const double unit = scaled / mean;
		const double t = floor(unit + 0.5);
		const u32 cell = t < 1.0 ? 1u : t > 65535.0 ? 65535u : (u32) t;
		table[i] = (uint16_t) cell;
		lo = std::min(lo, cell);
		hi = std::max(hi, cell);
	}
	if (info) { info->mean = mean; info->min_cost = lo; info->max_cost = hi; }
	return VDJX_OK;
}

extern "C" int vdjx_lineage_link(vdjx_ctx* c, const char* junctions, const uint64_t* off, const uint32_t* group, size_t n, const vdjx_lineage_link_params* prm,
                                 const uint16_t* table, int32_t* out_clone, int32_t* out_nearest, vdjx_lineage_info* info, vdjx_lineage_link_info* link) {
	if (info) memset(info, 0, sizeof *info);
	if (link) memset(link, 0, sizeof *link);
	if (!c || !prm) { vdjx_set_error("vdjx_lineage_link: NULL argument"); return VDJX_EINVAL; }
	if (prm->linkage < 0 || prm->linkage > 2) { vdjx_set_error("vdjx_lineage_link: linkage %d (0: single, 1: complete, 2: average)", prm->linkage); return VDJX_EINVAL; }
	if (table) {
		if (prm->symmetry != 0 && prm->symmetry != 1) { vdjx_set_error("vdjx_lineage_link: symmetry %d (0: avg, 1: min)", prm->symmetry); return VDJX_EINVAL; }
		for (u32 i = 0; i < LIN_TAB; i++)
			if (((i >> 6) & 3u) != (i & 3u) && table[i] == 0) {
				vdjx_set_error("vdjx_lineage_link: the table's cell [%u][%u] is 0 (an off-centre cell is 1 .. 65535)", i >> 2, i & 3u);
				return VDJX_EINVAL;
			}
	}
	return lin_run("vdjx_lineage_link", c, junctions, off, group, n, prm->num, prm->den, table, table ? (u32) prm->symmetry : 0u, out_clone, out_nearest, info,
	               prm->linkage, link);
}
