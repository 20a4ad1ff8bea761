// vdjx_nj.hip -- neighbour-joining lineage trees with inferred ancestors (gfx950 only, wave64).
//
//   vdjx_tree_nj   per lineage: the full matrix of window distances in 16.16 fixed point, neighbour joining under the strict order of the
//                  keys (Q, i, j), the tree rooted at the member of smallest (prio, index), the inferred nodes' sequences and every
//                  edge's mutations by Fitch parsimony (the model: include/vdjx.h; in Python: tests/tree_nj_model.py)
//   vdjx_nj_parents   (internal, vdjx_common.h) the same steps as far as the rooted parents, for vdjx_tree_mp's start
//
// The host sorts the keys, computes the windows and lays the members out as rows (vdjx_treelay.h, as vdjx_tree does), refuses a lineage of
// more than 4,096 members and cuts the lineages of two and more into batches of whole lineages of at most VDJX_NJ_CELLS matrix cells
// (vdjx_link.h's link_batches).  The rows are packed once; a batch is four dispatches:
//   k_nj_pack      a row = `words` {bases, mask} pairs in vdjx_hamming.h's format (once per call)
//   k_nj_matrix    one wave per work item (lineage, row block of 64 rows, column slice).  The loops are k_tree_min's -- up to 16 words a lane
//                  keeps its row in registers and the columns go through LDS in tiles, wider windows go by in chunks of 16 words against
//                  tiles of 8 columns -- but the body is this file's own (profiles/hamming_engine_refactor_check.md): it STORES d << 16
//                  for every cell, 0 on the diagonal.  The lane of row i writes cell (column, i): the matrix is symmetric, and so the 64
//                  lanes write 512 consecutive bytes.
//   k_nj_join      one workgroup per lineage.  Up to VDJX_NJ_LDS_MEMBERS members the matrix is copied into LDS (32 KiB: four workgroups
//                  of 256 threads per CU), beyond that the workgroup (1,024 threads) works on the batch's matrix in global memory; R,
//                  the active list and the node ids are in LDS either way.  Per join: every wave takes rows of the active list and its
//                  lanes the columns behind the row, each keeps its smallest (Q, i, j); shuffles inside the wave, one slot per wave in
//                  LDS, and every thread reads the block's minimum.  Then one row and column of D is rewritten and R follows by
//                  subtraction and addition (integers: exact); the new node's R is an integer atomicAdd in LDS (a sum: any order).  The
//                  loop runs r = m down to 4, a fixed count: no spin-wait, nothing waits for another workgroup.  The edges (a, b, length)
//                  go out in creation order.
//   k_nj_fitch     (vdjx_fitch.h, shared with vdjx_mp.hip) one wave per (lineage, 64 window columns), a lane per column: Fitch's up-pass
//                  over the inferred nodes in post-order, the down-pass back, then the leaves; a node's mutations by one integer
//                  atomicAdd per (node, wave).
// Between k_nj_join and k_nj_fitch only the edges come back: rooting them, the depths and the post-order are O(nodes) on the host
// (vdjx_nj_host.h).  No floating point.  Scratch comes from the context's workspace.
#include "vdjx_common.h"
#include "vdjx_fitch.h"
#include "vdjx_hamming.h"
#include "vdjx_link.h"
#include "vdjx_nj_host.h"
#include "vdjx_treelay.h"

#include <string.h>

typedef long long i64;

#define NJ_REG_WORDS 16                  // a row of up to 16 words (512 bases) stays in registers
#define NJ_TILE 512u                     // {bases, mask} pairs of a tile: 8 KiB, 64 columns of up to 8 words or 32 of up to 16
#define NJ_CH_COLS 8                     // the chunked path: columns per tile
#define NJ_SHIFT 16
#define NJ_LDS_M VDJX_NJ_LDS_MEMBERS
#define NJ_Q_NONE 0x7FFFFFFFFFFFFFFFll

static_assert(NJ_MAX_M == VDJX_NJ_MAX_MEMBERS, "the header's limit");
static_assert((size_t) NJ_LDS_M * NJ_LDS_M * 8 <= 32768, "four workgroups of the LDS path per CU");

struct NjLin { u64 doff; u32 first, m, eoff, pad; };                          // the matrix's first cell; the first row; members; the first edge
static_assert(sizeof(NjLin) == 24, "uploaded as it is");
// the user words of a lineage's work items: u[0] its first row, u[1] its first word, u[2] its NjLin

// one thread per {bases, mask} pair; ri[rows] is a sentinel whose wbase is the number of pairs
__global__ __launch_bounds__(256) void k_nj_pack(const char* __restrict__ contigs, const TreeRow* __restrict__ ri, u32 rows, u32 total, ulonglong2* __restrict__ out) {
	const u32 t = blockIdx.x * 256u + threadIdx.x;
	if (t >= total) return;
	u32 lo = 0, hi = rows;                              // the row r with ri[r].wbase <= t < ri[r + 1].wbase
	while (hi - lo > 1u) {
		const u32 mid = (lo + hi) / 2u;
		if (ri[mid].wbase <= t) lo = mid; else hi = mid;
	}
	const TreeRow q = ri[lo];
	out[t] = ham_pack_word([&](u32 pos) { return contigs[q.at + pos]; }, t - q.wbase, q.w);
}

// the register path: W words per row, tiles of NJ_TILE / W columns
template <int W>
__device__ inline void nj_item(const HamItem it, const ulonglong2* __restrict__ words, const NjLin q, i64* __restrict__ D, ulonglong2* tile) {
	constexpr u32 TC = W <= 8 ? 64u : 32u;
	const u32 lane = threadIdx.x, myrow = it.row0 + lane;
	const bool live = myrow < it.row_end;
	const u32 r = live ? myrow : it.row0;
	const ulonglong2* cw = words + it.u[1];
	u64 x[W], m[W];
#pragma unroll
	for (int w = 0; w < W; w++) {
		const ulonglong2 p = cw[(size_t) (r - q.first) * W + w];
		x[w] = p.x;
		m[w] = p.y;
	}
	i64* mine = D + q.doff + (myrow - q.first);          // cell (column, my row): + column * m
	for (u32 base = it.col0; base < it.col_end; base += TC) {
		const u32 nc = min(TC, it.col_end - base);
		const ulonglong2* src = cw + (size_t) (base - q.first) * W;
		for (u32 i = lane; i < nc * (u32) W; i += 64u) tile[i] = src[i];
		__syncthreads();
		for (u32 c = 0; c < nc; c++) {
			u32 d = 0;
#pragma unroll
			for (int w = 0; w < W; w++) d += ham_word(x[w], m[w], tile[c * (u32) W + w]);
			if (live) mine[(size_t) (base + c - q.first) * q.m] = base + c == myrow ? 0 : (i64) d << NJ_SHIFT;
		}
		__syncthreads();
	}
}

// the chunked path: any number of words, in chunks of 16 against tiles of 8 columns, a running distance per column
__device__ inline void nj_item_wide(const HamItem it, const ulonglong2* __restrict__ words, const NjLin q, i64* __restrict__ D, ulonglong2* tile) {
	const u32 lane = threadIdx.x, myrow = it.row0 + lane, W = it.words;
	const bool live = myrow < it.row_end;
	const u32 r = live ? myrow : it.row0;
	const ulonglong2* cw = words + it.u[1];
	const ulonglong2* mw = cw + (size_t) (r - q.first) * W;
	i64* mine = D + q.doff + (myrow - q.first);
	for (u32 base = it.col0; base < it.col_end; base += NJ_CH_COLS) {
		const u32 nc = min((u32) NJ_CH_COLS, it.col_end - base);
		u32 d[NJ_CH_COLS];
#pragma unroll
		for (int c = 0; c < NJ_CH_COLS; c++) d[c] = 0;
		for (u32 w0 = 0; w0 < W; w0 += NJ_REG_WORDS) {
			u64 x[NJ_REG_WORDS], m[NJ_REG_WORDS];
#pragma unroll
			for (int w = 0; w < NJ_REG_WORDS; w++) {
				const ulonglong2 p = w0 + (u32) w < W ? mw[w0 + (u32) w] : make_ulonglong2(0, 0);
				x[w] = p.x;
				m[w] = p.y;
			}
			for (u32 i = lane; i < NJ_CH_COLS * NJ_REG_WORDS; i += 64u) {
				const u32 c = i / NJ_REG_WORDS, w = w0 + i % NJ_REG_WORDS;
				tile[i] = c < nc && w < W ? cw[(size_t) (base + c - q.first) * W + w] : make_ulonglong2(0, 0);
			}
			__syncthreads();
#pragma unroll
			for (int c = 0; c < NJ_CH_COLS; c++)
#pragma unroll
				for (int w = 0; w < NJ_REG_WORDS; w++) d[c] += ham_word(x[w], m[w], tile[c * NJ_REG_WORDS + w]);
			__syncthreads();
		}
#pragma unroll
		for (int c = 0; c < NJ_CH_COLS; c++)
			if ((u32) c < nc && live) mine[(size_t) (base + (u32) c - q.first) * q.m] = base + (u32) c == myrow ? 0 : (i64) d[c] << NJ_SHIFT;
	}
}

// one wave per work item; the word count is the lineage's, so it is uniform
__global__ __launch_bounds__(64) void k_nj_matrix(const HamItem* __restrict__ items, const ulonglong2* __restrict__ words, const NjLin* __restrict__ lins,
                                                  i64* __restrict__ D) {
	__shared__ ulonglong2 tile[NJ_TILE];
	const HamItem it = items[blockIdx.x];
	const NjLin q = lins[it.u[2]];
	switch (it.words) {                                    // (W below is the case's constant: HAM_CASES_16 declares it)
		HAM_CASES_16(nj_item<W>(it, words, q, D, tile))
		default: nj_item_wide(it, words, q, D, tile); break;
	}
}

__device__ inline i64 nj_floor_div(i64 a, i64 b) {        // b > 0
	i64 q = a / b;
	if (a % b != 0 && a < 0) q--;
	return q;
}
__device__ inline i64 nj_half(i64 a) { return a >> 1; }   // floor(a / 2): the shift of a signed value is arithmetic

// a candidate: Q, the pair's node ids (smaller << 16 | larger: what ties are broken by) and its positions in the active list
struct NjBest { i64 q; u32 ij, pos; };
__device__ inline bool nj_less(const NjBest& a, const NjBest& b) { return a.q < b.q || (a.q == b.q && a.ij < b.ij); }

// one workgroup of T threads per lineage of which[]; IN_LDS: the matrix is copied into LDS first (m <= NJ_LDS_M)
template <int T, bool IN_LDS>
__global__ __launch_bounds__(T) void k_nj_join(const NjLin* __restrict__ lins, const u32* __restrict__ which, i64* D_all, u32* __restrict__ ea,
                                               u32* __restrict__ eb, i64* __restrict__ elen) {
	constexpr u32 CAP = IN_LDS ? NJ_LDS_M : NJ_MAX_M, NW = T / 64;
	__shared__ i64 sD[IN_LDS ? NJ_LDS_M * NJ_LDS_M : 1];
	__shared__ i64 R[CAP];
	__shared__ uint16_t act[CAP], nid[CAP];                // the active slots; the node id in every slot
	__shared__ i64 wq[NW];
	__shared__ u32 wij[NW], wpos[NW];
	__shared__ unsigned long long racc;
	const NjLin q = lins[which[blockIdx.x]];
	const u32 tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, m = q.m;
	if (m < 2u || m > CAP) return;                         // (cannot be: the host sorts the lineages by path)
	i64* gD = D_all + q.doff;
	u32* oa = ea + q.eoff;
	u32* ob = eb + q.eoff;
	i64* ol = elen + q.eoff;
	if (m == 2u) {
		if (tid == 0) { oa[0] = 0; ob[0] = 1; ol[0] = gD[1]; }
		return;
	}
	i64* D = IN_LDS ? sD : gD;
	if (IN_LDS)
		for (u32 i = tid; i < m * m; i += T) sD[i] = gD[i];
	for (u32 s = tid; s < m; s += T) { act[s] = (uint16_t) s; nid[s] = (uint16_t) s; }
	if (tid == 0) racc = 0;
	__syncthreads();
	for (u32 s = tid; s < m; s += T) {                     // (down the column: the matrix is symmetric, and the threads read side by side)
		i64 sum = 0;
		for (u32 k = 0; k < m; k++) sum += D[(size_t) k * m + s];
		R[s] = sum;
	}
	__syncthreads();
	u32 next = m;
	for (u32 r = m; r > 3u; r--) {
		NjBest b = {NJ_Q_NONE, 0xFFFFFFFFu, 0u};
		const i64 f = (i64) r - 2;
		for (u32 a = wave; a + 1u < r; a += NW) {
			const u32 sa = act[a], ia = nid[sa];
			const i64 Ra = R[sa];
			const i64* row = D + (size_t) sa * m;
			for (u32 c = a + 1u + lane; c < r; c += 64u) {
				const u32 sc = act[c], ic = nid[sc];
				const NjBest k = {f * row[sc] - Ra - R[sc], ia < ic ? ia << 16 | ic : ic << 16 | ia, a << 16 | c};
				if (nj_less(k, b)) b = k;
			}
		}
#pragma unroll
		for (int o = 32; o >= 1; o >>= 1) {
			const NjBest k = {(i64) vdjx_shfl_xor64((u64) b.q, o), (u32) __shfl_xor((int) b.ij, o, 64), (u32) __shfl_xor((int) b.pos, o, 64)};
			if (nj_less(k, b)) b = k;
		}
		if (lane == 0) { wq[wave] = b.q; wij[wave] = b.ij; wpos[wave] = b.pos; }
		__syncthreads();
		b = {wq[0], wij[0], wpos[0]};
		for (u32 w = 1; w < NW; w++) {
			const NjBest k = {wq[w], wij[w], wpos[w]};
			if (nj_less(k, b)) b = k;
		}
		// the pair: i the smaller node id, in slot si; j the larger, in slot sj at position pj of the active list
		const u32 pa = b.pos >> 16, pc = b.pos & 0xFFFFu, sa = act[pa], sc = act[pc];
		const bool a_first = nid[sa] < nid[sc];
		const u32 si = a_first ? sa : sc, sj = a_first ? sc : sa, pj = a_first ? pc : pa;
		const i64 dij = D[(size_t) si * m + sj], Ri = R[si], Rj = R[sj];
		const u32 last = act[r - 1u];
		__syncthreads();                                   // (everybody has read what the update overwrites)
		if (tid == 0) {
			const i64 bi = nj_floor_div(f * dij + Ri - Rj, 2 * f);
			const u32 e = 2u * (m - r);
			oa[e] = nid[si]; ob[e] = next; ol[e] = bi;
			oa[e + 1u] = nid[sj]; ob[e + 1u] = next; ol[e + 1u] = dij - bi;
		}
		i64 sum = 0;
		for (u32 a = tid; a < r; a += T) {
			const u32 sk = act[a];
			if (sk == si || sk == sj) continue;
			const i64 dik = D[(size_t) si * m + sk], djk = D[(size_t) sj * m + sk], nv = nj_half(dik + djk - dij);
			D[(size_t) si * m + sk] = nv;
			D[(size_t) sk * m + si] = nv;
			R[sk] += nv - dik - djk;
			sum += nv;
		}
		sum = (i64) vdjx_wave_sum64((u64) sum);
		if (lane == 0 && sum != 0) atomicAdd(&racc, (unsigned long long) sum);
		__syncthreads();
		if (tid == 0) {
			R[si] = (i64) racc;
			racc = 0;
			nid[si] = (uint16_t) next;
			act[pj] = (uint16_t) last;                       // (pj = r - 1: itself)
		}
		next++;
		__syncthreads();
	}
	if (tid == 0) {                                        // the last three meet in one more node
		u32 s[3] = {act[0], act[1], act[2]};
		for (int a = 0; a < 2; a++)
			for (int c = 0; c < 2 - a; c++)
				if (nid[s[c]] > nid[s[c + 1]]) { const u32 t = s[c]; s[c] = s[c + 1]; s[c + 1] = t; }
		const i64 dxy = D[(size_t) s[0] * m + s[1]], dxz = D[(size_t) s[0] * m + s[2]], dyz = D[(size_t) s[1] * m + s[2]];
		const i64 bx = nj_half(dxy + dxz - dyz);
		const u32 e = 2u * (m - 3u);
		oa[e] = nid[s[0]]; ob[e] = next; ol[e] = bx;
		oa[e + 1u] = nid[s[1]]; ob[e + 1u] = next; ol[e + 1u] = dxy - bx;
		oa[e + 2u] = nid[s[2]]; ob[e + 2u] = next; ol[e + 2u] = dxz - bx;
	}
}

extern "C" int vdjx_tree_nj_nodes(const int32_t* clone, size_t n, uint64_t* nodes) {
	if (!nodes || (n && !clone)) { vdjx_set_error("vdjx_tree_nj_nodes: NULL argument"); return VDJX_EINVAL; }
	if (!nj_count_nodes(clone, n, nodes)) { vdjx_set_error("vdjx_tree_nj_nodes: a clone below -1 (a key >= 0, or -1 for no part)"); return VDJX_EINVAL; }
	return VDJX_OK;
}

// vdjx_tree_nj behind its argument checks.  whole: the public call.  Not whole (vdjx_nj_parents): out_parent alone is written, the batch
// ends after the rooting, and no statistic is left
static int nj_run(vdjx_ctx* c, const char* who, const char* contigs, size_t n, int len, const int32_t* clone, const int32_t* anchor, const uint32_t* prio,
                  int32_t* out_parent, int64_t* out_length, int32_t* out_mutations, int32_t* out_depth, int32_t* out_clone, char* out_anc,
                  vdjx_tree_nj_info* info, const bool whole) {
	const auto t0 = std::chrono::steady_clock::now();
	std::vector<u64> keys;
	if (int rc = tree_keys(who, n, len, clone, anchor, keys)) return rc;
	const u32 rows = (u32) keys.size();
	TreeLay L;
	if (rows)
		if (int rc = tree_lay(who, keys, len, clone, anchor, prio, L)) return rc;
	vdjx_tree_nj_info inf;
	memset(&inf, 0, sizeof inf);
	inf.members = rows;
	inf.clones = (u32) L.clones.size();
	inf.largest_clone = L.largest;
	std::vector<u32> big, size;                            // the lineages of two and more: their index in L.clones, their members
	std::vector<u64> inf0(L.clones.size());                // per lineage: its first inferred node among the call's
	for (size_t k = 0; k < L.clones.size(); k++) {
		const TreeClone& q = L.clones[k];
		if (q.m > NJ_MAX_M) {
			vdjx_set_error("%s: clone %d has %u members (at most %u)", who, clone[L.row_item[q.first]], q.m, NJ_MAX_M);
			return VDJX_ELIMIT;
		}
		inf0[k] = inf.internal;
		if (q.m >= 2) { big.push_back((u32) k); size.push_back(q.m); inf.edges += 2ull * q.m - 3; inf.cells += (u64) q.m * q.m; }
		if (q.m >= 3) { inf.internal += q.m - 2; inf.joins += q.m - 3; }
	}
	const u64 nodes = (u64) n + inf.internal;
	for (u64 s = 0; s < nodes; s++) out_parent[s] = -1;
	if (whole)
		for (u64 s = 0; s < nodes; s++) {
			out_mutations[s] = out_depth[s] = out_clone[s] = -1;
			out_length[s] = -1;
		}
	if (out_anc) memset(out_anc, 0, (size_t) inf.internal * (size_t) len);
	for (const TreeClone& q : L.clones)
		if (whole && q.m == 1) {                              // a lone root
			const u32 i = L.row_item[q.first];
			out_depth[i] = 0;
			out_length[i] = 0;
			out_clone[i] = clone[i];
		}
	std::vector<u32> end;
	const u64 knob = (u64) vdjx_env_num("VDJX_NJ_CELLS", 1ll << 26, 1, 1ll << 28);
	link_batches(size, knob, end);
	inf.batches = (u32) end.size();
	if (!big.empty()) {
		HIP_TRY(hipSetDevice(c->device));
		hipStream_t st = c->stream;
		vdjx_work wk(c);
		char *d_contigs, *d_anc = nullptr;
		TreeRow* d_ri;
		ulonglong2* d_words;
		u32 *d_mut_row, *d_mut_inf, *d_leaf_par;
		HIP_TRY(wk.alloc(&d_contigs, n * (size_t) len));
		HIP_TRY(wk.alloc(&d_ri, (size_t) rows + 1));
		HIP_TRY(wk.alloc(&d_words, (size_t) L.total));
		HIP_TRY(wk.alloc(&d_mut_row, rows));
		HIP_TRY(wk.alloc(&d_mut_inf, inf.internal));
		HIP_TRY(wk.alloc(&d_leaf_par, rows));
		if (out_anc && inf.internal) {
			HIP_TRY(wk.alloc(&d_anc, (size_t) inf.internal * (size_t) len));
			HIP_TRY(hipMemsetAsync(d_anc, 0, (size_t) inf.internal * (size_t) len, st));
		}
		HIP_TRY(hipMemcpyAsync(d_contigs, contigs, n * (size_t) len, hipMemcpyHostToDevice, st));
		HIP_TRY(hipMemcpyAsync(d_ri, L.ri.data(), ((size_t) rows + 1) * sizeof(TreeRow), hipMemcpyHostToDevice, st));
		if (whole) {
			HIP_TRY(hipMemsetAsync(d_mut_row, 0, (size_t) rows * sizeof(u32), st));
			HIP_TRY(hipMemsetAsync(d_mut_inf, 0, (size_t) (inf.internal ? inf.internal : 1) * sizeof(u32), st));
		}
		{
			vdjx_prof_scope ps(c, "k_nj_pack");
			hipLaunchKernelGGL(k_nj_pack, dim3((u32) ((L.total + 255) / 256)), dim3(256), 0, st, (const char*) d_contigs, (const TreeRow*) d_ri, rows, (u32) L.total,
			                   d_words);
		}
		const vdjx_arena::mark_t mk = wk.mark();
		std::vector<NjLin> lins;
		std::vector<HamItem> items;
		std::vector<u32> in_lds, in_global, h_ea, h_eb, h_kid, h_par, h_order, leaf_par(rows, 0u);
		std::vector<i64> h_el;
		std::vector<NjFit> fits;
		std::vector<NjFitItem> fit_items;
		std::vector<NjTree> trees;
		NjTree t;
		for (size_t b = 0, k0 = 0; b < end.size(); k0 = end[b++]) {
			const size_t k1 = end[b], nl = k1 - k0;
			lins.clear(); items.clear(); in_lds.clear(); in_global.clear();
			u64 cells = 0, ne = 0;
			for (size_t k = k0; k < k1; k++) {
				const TreeClone& q = L.clones[big[k]];
				lins.push_back({cells, q.first, q.m, (u32) ne, 0u});
				(q.m <= NJ_LDS_M ? in_lds : in_global).push_back((u32) (k - k0));
				cells += (u64) q.m * q.m;
				ne += 2ull * q.m - 3;
			}
			const u32 slice = ham_slice_width(cells);
			for (size_t k = k0; k < k1; k++) {
				const TreeClone& q = L.clones[big[k]];
				ham_slice_items({q.first, q.m, q.words, {q.first, q.wbase, (u32) (k - k0)}}, slice, items);
			}
			NjLin* d_lins;
			HamItem* d_items;
			i64 *d_D, *d_el;
			u32 *d_which, *d_ea, *d_eb;
			HIP_TRY(wk.alloc(&d_lins, nl));
			HIP_TRY(wk.alloc(&d_items, items.size()));
			HIP_TRY(wk.alloc(&d_D, (size_t) cells));
			HIP_TRY(wk.alloc(&d_which, nl));
			HIP_TRY(wk.alloc(&d_ea, (size_t) ne));
			HIP_TRY(wk.alloc(&d_eb, (size_t) ne));
			HIP_TRY(wk.alloc(&d_el, (size_t) ne));
			HIP_TRY(hipMemcpyAsync(d_lins, lins.data(), nl * sizeof(NjLin), hipMemcpyHostToDevice, st));
			HIP_TRY(hipMemcpyAsync(d_items, items.data(), items.size() * sizeof(HamItem), hipMemcpyHostToDevice, st));
			if (!in_lds.empty()) HIP_TRY(hipMemcpyAsync(d_which, in_lds.data(), in_lds.size() * sizeof(u32), hipMemcpyHostToDevice, st));
			if (!in_global.empty())
				HIP_TRY(hipMemcpyAsync(d_which + in_lds.size(), in_global.data(), in_global.size() * sizeof(u32), hipMemcpyHostToDevice, st));
			{
				vdjx_prof_scope ps(c, "k_nj_matrix");
				hipLaunchKernelGGL(k_nj_matrix, dim3((u32) items.size()), dim3(64), 0, st, (const HamItem*) d_items, (const ulonglong2*) d_words, (const NjLin*) d_lins, d_D);
			}
			if (!in_lds.empty()) {
				vdjx_prof_scope ps(c, "k_nj_join_lds");
				hipLaunchKernelGGL((k_nj_join<256, true>), dim3((u32) in_lds.size()), dim3(256), 0, st, (const NjLin*) d_lins, (const u32*) d_which, d_D, d_ea, d_eb, d_el);
			}
			if (!in_global.empty()) {
				vdjx_prof_scope ps(c, "k_nj_join_global");
				hipLaunchKernelGGL((k_nj_join<1024, false>), dim3((u32) in_global.size()), dim3(1024), 0, st, (const NjLin*) d_lins,
				                   (const u32*) (d_which + in_lds.size()), d_D, d_ea, d_eb, d_el);
			}
			h_ea.resize((size_t) ne); h_eb.resize((size_t) ne); h_el.resize((size_t) ne);
			HIP_TRY(hipMemcpyAsync(h_ea.data(), d_ea, (size_t) ne * sizeof(u32), hipMemcpyDeviceToHost, st));
			HIP_TRY(hipMemcpyAsync(h_eb.data(), d_eb, (size_t) ne * sizeof(u32), hipMemcpyDeviceToHost, st));
			HIP_TRY(hipMemcpyAsync(h_el.data(), d_el, (size_t) ne * sizeof(i64), hipMemcpyDeviceToHost, st));
			HIP_TRY(hipStreamSynchronize(st));
			HIP_TRY(hipGetLastError());
			// the host's part: root every lineage, fill the outputs that need no sequence, lay the trees out for Fitch's passes
			fits.clear(); fit_items.clear(); h_kid.clear(); h_par.clear(); h_order.clear();
			u64 fs_bytes = 0;
			const u64 batch_inf0 = inf0[big[k0]];                // the batch's inferred nodes are a run of the call's
			for (size_t k = k0; k < k1; k++) {
				const TreeClone& q = L.clones[big[k]];
				const NjLin& l = lins[k - k0];
				const u32 m = q.m, root = q.root - q.first;
				if (!nj_orient(m, h_ea.data() + l.eoff, h_eb.data() + l.eoff, (const int64_t*) (h_el.data() + l.eoff), root, t)) {
					vdjx_set_error("%s: the %u edges of clone %d (%u members) are no tree", who, 2 * m - 3, clone[L.row_item[q.first]], m);
					return VDJX_ESTATE;
				}
				const u64 a0 = inf0[big[k]];
				auto slot = [&](u32 v) { return v < m ? (u64) L.row_item[q.first + v] : (u64) n + a0 + (v - m); };
				if (!whole) {
					for (u32 v = 0; v < (u32) t.parent.size(); v++) out_parent[slot(v)] = t.parent[v] < 0 ? -1 : (int32_t) slot((u32) t.parent[v]);
					continue;
				}
				for (u32 v = 0; v < (u32) t.parent.size(); v++) {
					const u64 s = slot(v);
					out_clone[s] = clone[L.row_item[q.first]];
					out_depth[s] = t.depth[v];
					out_length[s] = t.length[v];
					out_parent[s] = t.parent[v] < 0 ? -1 : (int32_t) slot((u32) t.parent[v]);
					if (t.parent[v] < 0) continue;
					inf.length += t.length[v];
					inf.negative += t.length[v] < 0;
					if (v < m) leaf_par[q.first + v] = (u32) t.parent[v];
					else h_par.push_back((u32) t.parent[v]);    // (v ascends: index node0 + v - m)
				}
				const u32 node0 = (u32) (a0 - batch_inf0);
				h_kid.insert(h_kid.end(), t.kid.begin(), t.kid.end());
				fits.push_back({fs_bytes, q.first, m, q.w, node0, root, t.root_kid, (u32) h_order.size(), 0u});
				h_order.insert(h_order.end(), t.order.begin(), t.order.end());
				for (u32 c0 = 0; c0 < q.w; c0 += 64u) fit_items.push_back({(u32) (k - k0), c0});
				fs_bytes += (u64) (m - 2u) * q.w;
			}
			if (!whole) {                                        // (the stream is idle: the edges' copies were waited for)
				vdjx_prof_collect(c, false);
				wk.release_to(mk);
				continue;
			}
			NjFit* d_fits;
			NjFitItem* d_fit_items;
			u32 *d_kid, *d_par, *d_order;
			uint8_t* d_fs;
			HIP_TRY(wk.alloc(&d_fits, fits.size()));
			HIP_TRY(wk.alloc(&d_fit_items, fit_items.size()));
			HIP_TRY(wk.alloc(&d_kid, h_kid.size()));
			HIP_TRY(wk.alloc(&d_par, h_par.size()));
			HIP_TRY(wk.alloc(&d_order, h_order.size()));
			HIP_TRY(wk.alloc(&d_fs, (size_t) fs_bytes));
			HIP_TRY(hipMemcpyAsync(d_fits, fits.data(), fits.size() * sizeof(NjFit), hipMemcpyHostToDevice, st));
			HIP_TRY(hipMemcpyAsync(d_fit_items, fit_items.data(), fit_items.size() * sizeof(NjFitItem), hipMemcpyHostToDevice, st));
			if (!h_kid.empty()) {
				HIP_TRY(hipMemcpyAsync(d_kid, h_kid.data(), h_kid.size() * sizeof(u32), hipMemcpyHostToDevice, st));
				HIP_TRY(hipMemcpyAsync(d_par, h_par.data(), h_par.size() * sizeof(u32), hipMemcpyHostToDevice, st));
				HIP_TRY(hipMemcpyAsync(d_order, h_order.data(), h_order.size() * sizeof(u32), hipMemcpyHostToDevice, st));
			}
			HIP_TRY(hipMemcpyAsync(d_leaf_par, leaf_par.data(), (size_t) rows * sizeof(u32), hipMemcpyHostToDevice, st));
			{
				vdjx_prof_scope ps(c, "k_nj_fitch");
				hipLaunchKernelGGL(k_nj_fitch, dim3((u32) fit_items.size()), dim3(64), 0, st, (const NjFitItem*) d_fit_items, (const NjFit*) d_fits, (const char*) d_contigs,
				                   (const TreeRow*) d_ri, (const u32*) d_kid, (const u32*) d_par, (const u32*) d_order, (const u32*) d_leaf_par, d_fs, d_mut_row,
				                   d_mut_inf + batch_inf0, d_anc ? d_anc + (size_t) batch_inf0 * (size_t) len : nullptr, (u32) len);
			}
			HIP_TRY(hipStreamSynchronize(st));                  // (the host vectors are uploaded from again, and the workspace is given up)
			HIP_TRY(hipGetLastError());
			vdjx_prof_collect(c, false);
			wk.release_to(mk);
		}
		if (!whole) return VDJX_OK;
		std::vector<u32> mut_row(rows), mut_inf((size_t) inf.internal);
		HIP_TRY(hipMemcpyAsync(mut_row.data(), d_mut_row, (size_t) rows * sizeof(u32), hipMemcpyDeviceToHost, st));
		if (inf.internal) HIP_TRY(hipMemcpyAsync(mut_inf.data(), d_mut_inf, (size_t) inf.internal * sizeof(u32), hipMemcpyDeviceToHost, st));
		if (d_anc) HIP_TRY(hipMemcpyAsync(out_anc, d_anc, (size_t) inf.internal * (size_t) len, hipMemcpyDeviceToHost, st));
		HIP_TRY(hipStreamSynchronize(st));
		for (u32 r = 0; r < rows; r++) {
			const u32 i = L.row_item[r];
			if (out_parent[i] < 0) continue;
			out_mutations[i] = (int32_t) mut_row[r];
			inf.parsimony += mut_row[r];
		}
		for (u64 a = 0; a < inf.internal; a++) {
			out_mutations[n + a] = (int32_t) mut_inf[a];
			inf.parsimony += mut_inf[a];
		}
	}
	if (!whole) return VDJX_OK;
	if (info) *info = inf;
	c->stats["tree_nj_cells"] = inf.cells;
	c->stats["tree_nj_joins"] = inf.joins;
	c->stats["tree_nj_us"] = (u64) std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
	return VDJX_OK;
}

extern "C" int vdjx_tree_nj(vdjx_ctx* c, const char* contigs, size_t n, int len, const int32_t* clone, const int32_t* anchor, const uint32_t* prio,
                            int32_t* out_parent, int64_t* out_length, int32_t* out_mutations, int32_t* out_depth, int32_t* out_clone, char* out_anc,
                            vdjx_tree_nj_info* info) {
	static const char* who = "vdjx_tree_nj";
	if (info) memset(info, 0, sizeof *info);
	if (!c) { vdjx_set_error("%s: NULL argument", who); return VDJX_EINVAL; }
	if (n == 0) return VDJX_OK;
	if (!contigs || !clone || !anchor || !out_parent || !out_length || !out_mutations || !out_depth || !out_clone) {
		vdjx_set_error("%s: NULL argument", who);
		return VDJX_EINVAL;
	}
	if (int rc = tree_check_contigs(who, contigs, n, len)) return rc;
	return nj_run(c, who, contigs, n, len, clone, anchor, prio, out_parent, out_length, out_mutations, out_depth, out_clone, out_anc, info, true);
}

int vdjx_nj_parents(vdjx_ctx* c, const char* contigs, size_t n, int len, const int32_t* clone, const int32_t* anchor, const uint32_t* prio,
                    int32_t* out_parent) {
	return nj_run(c, "vdjx_tree_nj", contigs, n, len, clone, anchor, prio, out_parent, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, false);
}
