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
#include "vdjx_common.h"
#include "vdjx_hamming.h"
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

// what vdjx_lineage and vdjx_lineage_model share: the checks, the host layout and every dispatch but the pair pass.  table == NULL: the
// Hamming pass; otherwise the caller's checked table, dmax in units of 2000 a position
static int lin_run(const char* fn, vdjx_ctx* c, const char* junctions, const uint64_t* off, const uint32_t* group, size_t n, int num, int den,
                   const uint16_t* table, u32 sym, int32_t* out_clone, int32_t* out_nearest, vdjx_lineage_info* info) {
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
