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
#include "vdjx_common.h"
#include "vdjx_hamming.h"
#include "vdjx_scan.h"
#include "vdjx_unionfind.h"

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

extern "C" int vdjx_lineage(vdjx_ctx* c, const char* junctions, const uint64_t* off, const uint32_t* group, size_t n, const vdjx_lineage_params* prm,
                            int32_t* out_clone, int32_t* out_nearest, vdjx_lineage_info* info) {
	if (info) memset(info, 0, sizeof *info);
	if (!c || !prm) { vdjx_set_error("vdjx_lineage: NULL argument"); return VDJX_EINVAL; }
	if (prm->den < 1 || prm->den > 1000000 || prm->num < 0 || prm->num > prm->den) {
		vdjx_set_error("vdjx_lineage: threshold %d/%d (den 1 .. 10^6, num 0 .. den)", prm->num, prm->den);
		return VDJX_EINVAL;
	}
	if (n == 0) return VDJX_OK;
	if (!junctions || !off || !group || !out_clone) { vdjx_set_error("vdjx_lineage: NULL argument"); return VDJX_EINVAL; }
	if (n >= (1ull << 20)) { vdjx_set_error("vdjx_lineage: %zu items (at most 2^20 - 1 per call)", n); return VDJX_EINVAL; }
	const auto t0 = std::chrono::steady_clock::now();
	std::vector<u64> keys;                                 // group << 28 | length << 20 | index: the bucket order
	for (size_t i = 0; i < n; i++) {
		if (off[i + 1] < off[i]) { vdjx_set_error("vdjx_lineage: offsets of item %zu decrease", i); return VDJX_EINVAL; }
		if (group[i] == VDJX_LINEAGE_NONE) continue;
		const u64 L = off[i + 1] - off[i];
		if (L == 0 || L > VDJX_LINEAGE_MAXLEN) {
			vdjx_set_error("vdjx_lineage: item %zu has %llu bases (1 .. %d)", i, (unsigned long long) L, VDJX_LINEAGE_MAXLEN);
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
		const u32 dmax = (u32) ((u64) prm->num * L / (u64) prm->den);      // d * den <= num * L  <=>  d <= floor(num * L / den)
		ham_slice_items({b.x, b.y, (L + 31u) / 32u, {dmax, 0u, 0u}}, slice, items);
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
	unsigned long long* d_links;
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
	HIP_TRY(wk.alloc(&d_links, 1));
	HIP_TRY(wk.alloc(&d_out, 2 * n));
	u32 *d_parent = d_state, *d_near = d_state + n;
	if (jbytes) HIP_TRY(hipMemcpyAsync(d_junc, junctions + off[0], jbytes, hipMemcpyHostToDevice, st));
	HIP_TRY(hipMemcpyAsync(d_ri, ri.data(), rows * sizeof(LinRow), hipMemcpyHostToDevice, st));
	HIP_TRY(hipMemcpyAsync(d_items, items.data(), items.size() * sizeof(HamItem), hipMemcpyHostToDevice, st));
	HIP_TRY(hipMemsetAsync(d_state, 0xFF, 2 * n * sizeof(u32), st));
	HIP_TRY(hipMemsetAsync(d_links, 0, sizeof(unsigned long long), st));
	const u32 nb = (u32) ((n + 255) / 256);
	{
		vdjx_prof_scope ps(c, "k_lin_pack");
		hipLaunchKernelGGL(k_lin_pack, dim3((rows * LIN_ROW_WORDS + 255u) / 256u), dim3(256), 0, st, (const char*) d_junc, (const LinRow*) d_ri, rows, d_rows,
		                   d_row_item, d_parent);
	}
	{
		vdjx_prof_scope ps(c, "k_lin_pairs");
		hipLaunchKernelGGL(k_lin_pairs, dim3((u32) items.size()), dim3(64), 0, st, (const HamItem*) d_items, (const ulonglong2*) d_rows,
		                   (const u32*) d_row_item, d_parent, d_near, d_links);
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
	unsigned long long links = 0;
	u32 clones = 0;
	HIP_TRY(hipMemcpyAsync(out_clone, d_out, n * sizeof(int32_t), hipMemcpyDeviceToHost, st));
	if (out_nearest) HIP_TRY(hipMemcpyAsync(out_nearest, d_out + n, n * sizeof(int32_t), hipMemcpyDeviceToHost, st));
	HIP_TRY(hipMemcpyAsync(&links, d_links, sizeof links, hipMemcpyDeviceToHost, st));
	HIP_TRY(hipMemcpyAsync(&clones, d_number + n, sizeof clones, hipMemcpyDeviceToHost, st));
	HIP_TRY(hipStreamSynchronize(st));
	HIP_TRY(hipGetLastError());
	vdjx_prof_collect(c, false);
	inf.links = links;
	inf.clones = clones;
	if (info) *info = inf;
	c->stats["lineage_work_items"] = items.size();
	c->stats["lineage_us"] = (u64) std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
	return VDJX_OK;
}
