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
//
//   vdjx_tree_split_support   the delete-half jackknife around the joining: how many replicates' trees have the split (bipartition) of
//                  every inferred node of a caller's tree.  A unit is one (replicate, lineage of four and more) and one NjLin, so
//                  k_nj_matrix and k_nj_join run as they are, on rows of the kept columns; around them
//   k_split_pack   k_nj_pack through a replicate's list of kept window positions
//   k_split_clades one wave per unit, a lane per 64-bit word: the clade of every join as the union of two earlier ones, canonical (the side
//                  without the root member), with its signature
//   k_split_match  one wave per unit, a lane per clade: a binary search among the scored tree's sorted signatures, all words compared, one
//                  integer atomicAdd per hit
//   vdjx_tree_split_compare   the match step on the host (vdjx_split_host.h), for two trees of a caller's
#include "vdjx_common.h"
#include "vdjx_fitch.h"
#include "vdjx_hamming.h"
#include "vdjx_link.h"
#include "vdjx_nj_host.h"
#include "vdjx_split_host.h"
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

// ---- vdjx_tree_split_support's own kernels: the jackknife's pack, the clades of a join order, their look-up among the scored clades ----

// a scored lineage (four and more members): where its scored clades and signatures start, how many they are
struct SplitLin { u64 cbase; u32 m, root, words, nsc, soff, pad; };            // cbase: its first word in sclade[]; soff: its first entry in ssig[] / sslot[]
// a unit (replicate, lineage) of a batch -- unit u is also lins[u]: where its clades and signatures go, which scored lineage it is
struct SplitUnit { u64 woff; u32 joff, lin; };
static_assert(sizeof(SplitLin) == 32 && sizeof(SplitUnit) == 16, "uploaded as they are");

// k_nj_pack with selection: row r's characters are the kept window positions of replicate row_rep[r] (sel: `stride` ascending positions per
// replicate, of which the row uses its first q.w).  A row that keeps nothing is one word of zeros
__global__ __launch_bounds__(256) void k_split_pack(const char* __restrict__ contigs, const TreeRow* __restrict__ ri, u32 rows, u32 total,
                                                    const uint16_t* __restrict__ sel, u32 stride, const u32* __restrict__ row_rep, ulonglong2* __restrict__ out) {
	const u32 t = blockIdx.x * 256u + threadIdx.x;
	if (t >= total) return;
	u32 lo = 0, hi = rows;                              // the row r with ri[r].wbase <= t < ri[r + 1].wbase
	while (hi - lo > 1u) {
		const u32 mid = (lo + hi) / 2u;
		if (ri[mid].wbase <= t) lo = mid; else hi = mid;
	}
	const TreeRow q = ri[lo];
	const uint16_t* mine = sel + (size_t) row_rep[lo] * stride;
	out[t] = ham_pack_word([&](u32 pos) { return contigs[q.at + mine[pos]]; }, t - q.wbase, q.w);
}

// One wave per unit, a lane per 64-bit word of a clade.  k_nj_join wrote the pairs (child, new node) in creation order: join j made node
// m + j of ea[2j] and ea[2j + 1], both of smaller id, so one pass builds every clade as the union of two earlier ones; the node where the
// last three meet is dropped.  A lane only ever reads the words it wrote itself: the chain needs no barrier.  Then a clade that holds the
// root's bit is complemented within m bits, and its signature follows (a sum over disjoint leaves: the children's sums; the complement's
// is the total minus it).  Up to 64 members a clade is one word, the chain is lane 0's in LDS and the word is its own signature.
__global__ __launch_bounds__(64) void k_split_clades(const NjLin* __restrict__ lins, const SplitUnit* __restrict__ units, const SplitLin* __restrict__ slins,
                                                     const u32* __restrict__ ea, u64* clades, u64* sigs) {
	__shared__ u64 one[NJ_LDS_M];                          // 512 bytes: the wave limit (32 workgroups of one wave per CU) binds long before LDS does
	static_assert(sizeof(u64) * NJ_LDS_M * 32 <= 160 * 1024, "32 workgroups per CU");
	const u32 lane = threadIdx.x;
	const NjLin q = lins[blockIdx.x];
	const SplitUnit su = units[blockIdx.x];
	const SplitLin s = slins[su.lin];
	const u32 m = q.m, words = s.words;
	if (m < 4u || m > NJ_MAX_M || words != (m + 63u) / 64u || s.root >= m) return;      // (cannot be: the host lays out lineages of four and more)
	const u32 nj = m - 3u;
	const u32* kid = ea + q.eoff;
	u64* out = clades + su.woff;
	u64* sg = sigs + su.joff;
	if (words == 1u) {
		if (lane == 0)
			for (u32 j = 0; j < nj; j++) {
				const u32 a = kid[2u * j], b = kid[2u * j + 1u];
				const u64 wa = a < m ? 1ull << a : a - m < j ? one[a - m] : 0ull, wb = b < m ? 1ull << b : b - m < j ? one[b - m] : 0ull;
				one[j] = wa | wb;
			}
		__syncthreads();
		if (lane < nj) {
			u64 w = one[lane];
			if (w >> s.root & 1u) w = ~w & (m == 64u ? ~0ull : (1ull << m) - 1ull);
			out[lane] = w;
			sg[lane] = w;
		}
		return;
	}
	u64 total = 0;
	for (u32 v = lane; v < m; v += 64u) total += vdjx_mix64((u64) v + 1u);
	total = vdjx_wave_sum64(total);
	const bool mine = lane < words;
	for (u32 j = 0; j < nj; j++) {
		const u32 a = kid[2u * j], b = kid[2u * j + 1u];     // (a - m < j: an earlier join -- anything else reads nothing)
		const u64 wa = a < m ? ((a >> 6) == lane ? 1ull << (a & 63u) : 0ull) : mine && a - m < j ? out[(size_t) (a - m) * words + lane] : 0ull;
		const u64 wb = b < m ? ((b >> 6) == lane ? 1ull << (b & 63u) : 0ull) : mine && b - m < j ? out[(size_t) (b - m) * words + lane] : 0ull;
		if (mine) out[(size_t) j * words + lane] = wa | wb;
		if (lane == 0) {
			const u64 sa = a < m ? vdjx_mix64((u64) a + 1u) : a - m < j ? sg[a - m] : 0ull, sb = b < m ? vdjx_mix64((u64) b + 1u) : b - m < j ? sg[b - m] : 0ull;
			sg[j] = sa + sb;
		}
	}
	const u64 last = (m & 63u) ? (1ull << (m & 63u)) - 1ull : ~0ull;
	for (u32 j = 0; j < nj; j++) {
		const u64 w = mine ? out[(size_t) j * words + lane] : 0ull;
		const bool flip = __ballot(lane == (s.root >> 6) && (w >> (s.root & 63u) & 1u)) != 0;
		if (!flip) continue;
		if (mine) out[(size_t) j * words + lane] = lane + 1u == words ? ~w & last : ~w;
		if (lane == 0) sg[j] = total - sg[j];
	}
}

// One wave per unit, a lane per clade: the clade is looked up among its lineage's scored clades -- a binary search over the sorted signatures,
// then the run of equal ones -- and counts only where every word is equal: one integer atomicAdd on the scored node's counter
__global__ __launch_bounds__(64) void k_split_match(const NjLin* __restrict__ lins, const SplitUnit* __restrict__ units, const SplitLin* __restrict__ slins,
                                                    const u64* __restrict__ clades, const u64* __restrict__ sigs, const u64* __restrict__ ssig,
                                                    const u64* __restrict__ sclade, const u32* __restrict__ sslot, u32* support) {
	const NjLin q = lins[blockIdx.x];
	const SplitUnit su = units[blockIdx.x];
	const SplitLin s = slins[su.lin];
	if (q.m < 4u || q.m != s.m) return;                    // (cannot be)
	const u32 nj = q.m - 3u, words = s.words;
	const u64* key = ssig + s.soff;
	for (u32 j = threadIdx.x; j < nj; j += 64u) {
		const u64 sig = sigs[su.joff + j];
		const u64* mine = clades + su.woff + (size_t) j * words;
		u32 lo = 0, hi = s.nsc;                              // the first scored clade whose signature is not below sig
		while (lo < hi) {
			const u32 mid = (lo + hi) / 2u;
			if (key[mid] < sig) lo = mid + 1u; else hi = mid;
		}
		for (u32 i = lo; i < s.nsc && key[i] == sig; i++) {
			const u64* theirs = sclade + s.cbase + (size_t) i * words;
			bool same = true;
			for (u32 l = 0; l < words && same; l++) same = mine[l] == theirs[l];
			if (same) { atomicAdd(support + sslot[s.soff + i], 1u); break; }
		}
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

// what both split calls do with a caller's tree of one lineage: its nodes' local parents checked and rooted, the scored clades canonical
static int split_check(const char* who, const char* what, const int32_t* parent, size_t n, const int32_t* item_row, const u32* row_item, const int32_t* clone,
                       u32 first, u32 m, u64 a0, u32 root, std::vector<int32_t>& lp, NjTree& t) {
	if (const int e = split_lineage(parent, n, item_row, row_item, first, m, a0, root, lp, t)) {
		vdjx_set_error("%s: %s of clone %d (%u members) are no tree: %s", who, what, clone[row_item[first]], m, mp_why(e));
		return VDJX_EINVAL;
	}
	return VDJX_OK;
}

// vdjx_tree_split_support -- the delete-half jackknife around neighbour joining.  The host lays the lineages out as nj_run does, checks the
// scored tree (mp_local, mp_orient), makes its canonical clades per lineage of four and more and every replicate's kept positions, and cuts
// the (replicate, lineage) units, replicate-major, into batches of at most VDJX_NJ_CELLS matrix cells.  A batch is k_split_pack, k_nj_matrix
// and k_nj_join as they are (a unit is an NjLin), k_split_clades and k_split_match; nothing is read back unless the replicates' trees are
// asked for.  The supports come back once.
extern "C" int vdjx_tree_split_support(vdjx_ctx* c, const char* contigs, size_t n, int len, const int32_t* clone, const int32_t* anchor, const uint32_t* prio,
                                       const int32_t* parent, const vdjx_tree_split_params* params, int32_t* out_support, int32_t* out_rep_parent,
                                       vdjx_tree_split_info* info) {
	static const char* who = "vdjx_tree_split_support";
	if (info) memset(info, 0, sizeof *info);
	if (!c) { vdjx_set_error("%s: NULL argument", who); return VDJX_EINVAL; }
	if (n == 0) return VDJX_OK;
	if (!contigs || !clone || !anchor || !params) { vdjx_set_error("%s: NULL argument", who); return VDJX_EINVAL; }
	if (!parent) { vdjx_set_error("%s: NULL argument (parent)", who); return VDJX_EINVAL; }
	if (!out_support) { vdjx_set_error("%s: NULL argument (out_support)", who); return VDJX_EINVAL; }
	if (params->replicates < 1 || params->replicates > 1024) { vdjx_set_error("%s: %u replicates (1 .. 1024)", who, params->replicates); return VDJX_EINVAL; }
	if (params->reserved != 0) { vdjx_set_error("%s: params->reserved is %u (must be 0)", who, params->reserved); return VDJX_EINVAL; }
	if (int rc = tree_check_contigs(who, contigs, n, len)) return rc;
	const auto t0 = std::chrono::steady_clock::now();
	const u32 B = params->replicates;
	std::vector<u64> keys;
	if (int rc = tree_keys(who, n, len, clone, anchor, keys)) return rc;
	const u32 rows = (u32) keys.size();
	TreeLay L;
	if (rows)
		if (int rc = tree_lay(who, keys, len, clone, anchor, prio, L)) return rc;
	vdjx_tree_split_info inf;
	memset(&inf, 0, sizeof inf);
	inf.members = rows;
	inf.clones = (u32) L.clones.size();
	inf.largest_clone = L.largest;
	inf.replicates = B;
	std::vector<u64> inf0(L.clones.size());                // per lineage: its first inferred node among the call's
	u64 internal = 0;
	for (size_t k = 0; k < L.clones.size(); k++) {
		const TreeClone& q = L.clones[k];
		if (q.m > NJ_MAX_M) {
			vdjx_set_error("%s: clone %d has %u members (at most %u)", who, clone[L.row_item[q.first]], q.m, NJ_MAX_M);
			return VDJX_ELIMIT;
		}
		inf0[k] = internal;
		if (q.m >= 3) internal += q.m - 2;
	}
	const u64 nodes = (u64) n + internal;
	// the scored tree: every lineage checked as vdjx_tree_mp checks a start; of the lineages of four and more the canonical clades of the
	// scored nodes, sorted by signature
	std::vector<int32_t> item_row(n, -1), lp;
	for (u32 r = 0; r < rows; r++) item_row[L.row_item[r]] = (int32_t) r;
	std::vector<u32> big;                                  // the lineages of four and more: their index in L.clones
	std::vector<SplitLin> slins;
	std::vector<u64> ssig, sclade;
	std::vector<uint64_t> cl;
	std::vector<u32> sslot;                                // a scored clade's counter: its node among the call's inferred nodes
	std::vector<SplitScored> sc;
	std::vector<uint8_t> scored((size_t) internal, 0);
	NjTree t;
	u32 maxw = 0;
	u64 unit_cells = 0;
	for (size_t k = 0; k < L.clones.size(); k++) {
		const TreeClone& q = L.clones[k];
		const u32 m = q.m, root = q.root - q.first;
		if (int rc = split_check(who, "the parents", parent, n, item_row.data(), L.row_item.data(), clone, q.first, m, inf0[k], root, lp, t)) return rc;
		if (m < 4) continue;
		const u32 words = split_words(m);
		split_clades(m, t, cl);
		split_scored(m, root, t.root_kid, cl, sc);
		slins.push_back({(u64) sclade.size(), m, root, words, (u32) sc.size(), (u32) ssig.size(), 0u});
		for (const SplitScored& x : sc) {
			ssig.push_back(x.sig);
			sslot.push_back((u32) (inf0[k] + (x.node - m)));
			sclade.insert(sclade.end(), cl.begin() + (size_t) (x.node - m) * words, cl.begin() + (size_t) (x.node - m + 1) * words);
			scored[(size_t) (inf0[k] + (x.node - m))] = 1;
		}
		big.push_back((u32) k);
		maxw = std::max(maxw, q.w);
		unit_cells += (u64) m * m;
		inf.scored += m - 3;
	}
	for (u64 s = 0; s < nodes; s++) out_support[s] = s >= n && scored[(size_t) (s - n)] ? 0 : -1;
	inf.units = B * (u32) big.size();                      // (below 2^10 * 2^18)
	inf.joins = (u64) B * inf.scored;
	inf.cells = (u64) B * unit_cells;
	if (out_rep_parent) {                                  // the lineages of three and fewer have one tree whatever the distances are
		for (u64 s = 0; s < (u64) B * nodes; s++) out_rep_parent[s] = -1;
		for (size_t k = 0; k < L.clones.size(); k++) {
			const TreeClone& q = L.clones[k];
			if (q.m < 2 || q.m > 3) continue;
			const int32_t root = (int32_t) L.row_item[q.root], top = q.m == 3 ? (int32_t) (n + inf0[k]) : root;
			for (u32 r = 0; r < B; r++) {
				int32_t* row = out_rep_parent + (size_t) r * nodes;
				for (u32 v = 0; v < q.m; v++)
					if (q.first + v != q.root) row[L.row_item[q.first + v]] = top;
				if (q.m == 3) row[top] = root;
			}
		}
	}
	// the units, replicate-major; unit x is replicate x / big.size() + 1 of lineage big[x % big.size()]
	std::vector<u32> size, end;
	size.reserve((size_t) inf.units);
	for (u32 r = 0; r < B; r++)
		for (const u32 k : big) size.push_back(L.clones[k].m);
	const u64 knob = (u64) vdjx_env_num("VDJX_NJ_CELLS", 1ll << 26, 1, 1ll << 28);
	link_batches(size, knob, end);
	inf.batches = (u32) end.size();
	if (!big.empty()) {
		const size_t nb = big.size();
		// every replicate's kept positions below the widest window, ascending, and how many lie below each lineage's w
		std::vector<uint16_t> sel((size_t) B * maxw, 0);
		std::vector<u32> kept(B, 0);
		for (u32 r = 0; r < B; r++) {
			uint16_t* mine = sel.data() + (size_t) r * maxw;
			u64 bits = 0;
			for (u32 q = 0; q < maxw; q++) {
				if ((q & 31u) == 0) bits = vdjx_mix64(params->seed ^ ((u64) (r + 1) << 32 | (u64) (q >> 5)));      // replicates count from 1
				if (bits >> (q & 31u) & 1u) mine[kept[r]++] = (uint16_t) q;
			}
		}
		HIP_TRY(hipSetDevice(c->device));
		hipStream_t st = c->stream;
		vdjx_work wk(c);
		char* d_contigs;
		uint16_t* d_sel;
		SplitLin* d_slins;
		u64 *d_ssig, *d_sclade;
		u32 *d_sslot, *d_support;
		HIP_TRY(wk.alloc(&d_contigs, n * (size_t) len));
		HIP_TRY(wk.alloc(&d_sel, sel.size()));
		HIP_TRY(wk.alloc(&d_slins, nb));
		HIP_TRY(wk.alloc(&d_ssig, ssig.size()));
		HIP_TRY(wk.alloc(&d_sclade, sclade.size()));
		HIP_TRY(wk.alloc(&d_sslot, sslot.size()));
		HIP_TRY(wk.alloc(&d_support, (size_t) internal));
		HIP_TRY(hipMemcpyAsync(d_contigs, contigs, n * (size_t) len, hipMemcpyHostToDevice, st));
		HIP_TRY(hipMemcpyAsync(d_sel, sel.data(), sel.size() * sizeof(uint16_t), hipMemcpyHostToDevice, st));
		HIP_TRY(hipMemcpyAsync(d_slins, slins.data(), nb * sizeof(SplitLin), hipMemcpyHostToDevice, st));
		HIP_TRY(hipMemcpyAsync(d_ssig, ssig.data(), ssig.size() * sizeof(u64), hipMemcpyHostToDevice, st));
		HIP_TRY(hipMemcpyAsync(d_sclade, sclade.data(), sclade.size() * sizeof(u64), hipMemcpyHostToDevice, st));
		HIP_TRY(hipMemcpyAsync(d_sslot, sslot.data(), sslot.size() * sizeof(u32), hipMemcpyHostToDevice, st));
		HIP_TRY(hipMemsetAsync(d_support, 0, (size_t) internal * sizeof(u32), st));
		const vdjx_arena::mark_t mk = wk.mark();
		std::vector<NjLin> lins;
		std::vector<SplitUnit> units;
		std::vector<HamItem> items;
		std::vector<TreeRow> ri;
		std::vector<u32> row_rep, in_lds, in_global, h_ea, h_eb;
		std::vector<int64_t> no_length;
		for (size_t b = 0, x0 = 0; b < end.size(); x0 = end[b++]) {
			const size_t x1 = end[b], nu = x1 - x0;
			lins.clear(); units.clear(); items.clear(); ri.clear(); row_rep.clear(); in_lds.clear(); in_global.clear();
			u64 cells = 0, ne = 0, total = 0, cw = 0, cj = 0;
			for (size_t x = x0; x < x1; x++) {
				const u32 r = (u32) (x / nb), l = (u32) (x % nb);
				const TreeClone& q = L.clones[big[l]];
				const uint16_t* mine = sel.data() + (size_t) r * maxw;
				const u32 kw = (u32) (std::lower_bound(mine, mine + kept[r], (uint16_t) q.w) - mine);      // kept positions below the lineage's w (w < 4096)
				const u32 words = std::max(1u, (kw + 31u) / 32u), first = (u32) ri.size();
				if (total + (u64) q.m * words > 0xFFFFFFFFull) { vdjx_set_error("%s: more than 2^32 packed words in a batch", who); return VDJX_ELIMIT; }
				for (u32 p = 0; p < q.m; p++) {
					ri.push_back({L.ri[q.first + p].at, (u32) total + p * words, kw});
					row_rep.push_back(r);
				}
				lins.push_back({cells, first, q.m, (u32) ne, 0u});
				units.push_back({cw, (u32) cj, l});
				(q.m <= NJ_LDS_M ? in_lds : in_global).push_back((u32) (x - x0));
				cells += (u64) q.m * q.m;
				ne += 2ull * q.m - 3;
				total += (u64) q.m * words;
				cw += (u64) (q.m - 3u) * split_words(q.m);
				cj += q.m - 3u;
			}
			if (ne > 0xFFFFFFFFull || cj > 0xFFFFFFFFull) { vdjx_set_error("%s: more than 2^32 edges in a batch", who); return VDJX_ELIMIT; }
			const u32 brows = (u32) ri.size();
			ri.push_back({0, (u32) total, 0});
			const u32 slice = ham_slice_width(cells);
			for (size_t x = x0; x < x1; x++) {
				const NjLin& l = lins[x - x0];
				const u32 words = (ri[l.first + 1u].wbase - ri[l.first].wbase);      // (a unit has four rows and more: the next row is its own)
				ham_slice_items({l.first, l.m, words, {l.first, ri[l.first].wbase, (u32) (x - x0)}}, slice, items);
			}
			TreeRow* d_ri;
			NjLin* d_lins;
			SplitUnit* d_units;
			HamItem* d_items;
			ulonglong2* d_words;
			i64 *d_D, *d_el;
			u32 *d_row_rep, *d_which, *d_ea, *d_eb;
			u64 *d_clades, *d_sigs;
			HIP_TRY(wk.alloc(&d_ri, (size_t) brows + 1));
			HIP_TRY(wk.alloc(&d_row_rep, brows));
			HIP_TRY(wk.alloc(&d_lins, nu));
			HIP_TRY(wk.alloc(&d_units, nu));
			HIP_TRY(wk.alloc(&d_items, items.size()));
			HIP_TRY(wk.alloc(&d_words, (size_t) total));
			HIP_TRY(wk.alloc(&d_D, (size_t) cells));
			HIP_TRY(wk.alloc(&d_which, nu));
			HIP_TRY(wk.alloc(&d_ea, (size_t) ne));
			HIP_TRY(wk.alloc(&d_eb, (size_t) ne));
			HIP_TRY(wk.alloc(&d_el, (size_t) ne));
			HIP_TRY(wk.alloc(&d_clades, (size_t) cw));
			HIP_TRY(wk.alloc(&d_sigs, (size_t) cj));
			HIP_TRY(hipMemcpyAsync(d_ri, ri.data(), ((size_t) brows + 1) * sizeof(TreeRow), hipMemcpyHostToDevice, st));
			HIP_TRY(hipMemcpyAsync(d_row_rep, row_rep.data(), (size_t) brows * sizeof(u32), hipMemcpyHostToDevice, st));
			HIP_TRY(hipMemcpyAsync(d_lins, lins.data(), nu * sizeof(NjLin), hipMemcpyHostToDevice, st));
			HIP_TRY(hipMemcpyAsync(d_units, units.data(), nu * sizeof(SplitUnit), hipMemcpyHostToDevice, st));
			HIP_TRY(hipMemcpyAsync(d_items, items.data(), items.size() * sizeof(HamItem), hipMemcpyHostToDevice, st));
			if (!in_lds.empty()) HIP_TRY(hipMemcpyAsync(d_which, in_lds.data(), in_lds.size() * sizeof(u32), hipMemcpyHostToDevice, st));
			if (!in_global.empty())
				HIP_TRY(hipMemcpyAsync(d_which + in_lds.size(), in_global.data(), in_global.size() * sizeof(u32), hipMemcpyHostToDevice, st));
			{
				vdjx_prof_scope ps(c, "k_split_pack");
				hipLaunchKernelGGL(k_split_pack, dim3((u32) ((total + 255) / 256)), dim3(256), 0, st, (const char*) d_contigs, (const TreeRow*) d_ri, brows, (u32) total,
				                   (const uint16_t*) d_sel, maxw, (const u32*) d_row_rep, d_words);
			}
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
			{
				vdjx_prof_scope ps(c, "k_split_clades");
				hipLaunchKernelGGL(k_split_clades, dim3((u32) nu), dim3(64), 0, st, (const NjLin*) d_lins, (const SplitUnit*) d_units, (const SplitLin*) d_slins,
				                   (const u32*) d_ea, d_clades, d_sigs);
			}
			{
				vdjx_prof_scope ps(c, "k_split_match");
				hipLaunchKernelGGL(k_split_match, dim3((u32) nu), dim3(64), 0, st, (const NjLin*) d_lins, (const SplitUnit*) d_units, (const SplitLin*) d_slins,
				                   (const u64*) d_clades, (const u64*) d_sigs, (const u64*) d_ssig, (const u64*) d_sclade, (const u32*) d_sslot, d_support);
			}
			if (out_rep_parent) {
				h_ea.resize((size_t) ne); h_eb.resize((size_t) ne);
				HIP_TRY(hipMemcpyAsync(h_ea.data(), d_ea, (size_t) ne * sizeof(u32), hipMemcpyDeviceToHost, st));
				HIP_TRY(hipMemcpyAsync(h_eb.data(), d_eb, (size_t) ne * sizeof(u32), hipMemcpyDeviceToHost, st));
			}
			HIP_TRY(hipStreamSynchronize(st));                  // (the host vectors are filled again, and the workspace is given up)
			HIP_TRY(hipGetLastError());
			if (out_rep_parent)
				for (size_t x = x0; x < x1; x++) {
					const u32 r = (u32) (x / nb), k = big[x % nb];
					const TreeClone& q = L.clones[k];
					const NjLin& l = lins[x - x0];
					const u32 m = q.m;
					no_length.assign(2 * (size_t) m - 3, 0);        // (the replicates' branch lengths are not computed)
					if (!nj_orient(m, h_ea.data() + l.eoff, h_eb.data() + l.eoff, no_length.data(), q.root - q.first, t)) {
						vdjx_set_error("%s: replicate %u: the %u edges of clone %d (%u members) are no tree", who, r + 1, 2 * m - 3, clone[L.row_item[q.first]], m);
						return VDJX_ESTATE;
					}
					int32_t* row = out_rep_parent + (size_t) r * nodes;
					auto slot = [&](u32 v) { return v < m ? (u64) L.row_item[q.first + v] : (u64) n + inf0[k] + (v - m); };
					for (u32 v = 0; v < (u32) t.parent.size(); v++) row[slot(v)] = t.parent[v] < 0 ? -1 : (int32_t) slot((u32) t.parent[v]);
				}
			vdjx_prof_collect(c, false);
			wk.release_to(mk);
		}
		std::vector<u32> support((size_t) internal);
		HIP_TRY(hipMemcpyAsync(support.data(), d_support, (size_t) internal * sizeof(u32), hipMemcpyDeviceToHost, st));
		HIP_TRY(hipStreamSynchronize(st));
		for (u64 a = 0; a < internal; a++) {
			if (!scored[(size_t) a]) continue;
			if (support[(size_t) a] > B) {
				vdjx_set_error("%s: node %llu counted in %u of %u replicates", who, (unsigned long long) (n + a), support[(size_t) a], B);
				return VDJX_ESTATE;
			}
			out_support[n + a] = (int32_t) support[(size_t) a];
			inf.matched += support[(size_t) a];
			inf.full += support[(size_t) a] == B;
		}
	}
	if (info) *info = inf;
	c->stats["tree_split_units"] = inf.units;
	c->stats["tree_split_batches"] = inf.batches;
	c->stats["tree_split_us"] = (u64) std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
	return VDJX_OK;
}

// vdjx_tree_split_compare -- the match step on the host, exactly: which scored clades of tree a tree b has.  The lineages and the slots are
// vdjx_tree_nj's; a lineage's root in a tree is its member without a parent, and both trees' clades are taken against tree a's root
extern "C" int vdjx_tree_split_compare(const int32_t* clone, size_t n, const int32_t* parent_a, const int32_t* parent_b, uint64_t nodes, int32_t* out_shared,
                                       uint64_t* shared, uint64_t* scored) {
	static const char* who = "vdjx_tree_split_compare";
	if (shared) *shared = 0;
	if (scored) *scored = 0;
	if (n == 0 && nodes == 0) return VDJX_OK;
	if (!clone || !parent_a || !parent_b || !out_shared) { vdjx_set_error("%s: NULL argument", who); return VDJX_EINVAL; }
	if (n >= (1ull << 20)) { vdjx_set_error("%s: %zu items (at most 2^20 - 1 per call)", who, n); return VDJX_EINVAL; }
	uint64_t want = 0;
	if (!nj_count_nodes(clone, n, &want)) { vdjx_set_error("%s: a clone below -1 (a key >= 0, or -1 for no part)", who); return VDJX_EINVAL; }
	if (want != nodes) { vdjx_set_error("%s: %llu nodes, but the clones of the %zu items make %llu", who, (unsigned long long) nodes, n, (unsigned long long) want); return VDJX_EINVAL; }
	std::vector<u64> keys;
	for (size_t i = 0; i < n; i++)
		if (clone[i] >= 0) keys.push_back((u64) (u32) clone[i] << 20 | (u64) i);
	std::sort(keys.begin(), keys.end());
	const u32 rows = (u32) keys.size();
	std::vector<int32_t> item_row(n, -1), lp;
	std::vector<u32> row_item(rows);
	for (u32 r = 0; r < rows; r++) { row_item[r] = (u32) (keys[r] & 0xFFFFFu); item_row[row_item[r]] = (int32_t) r; }
	for (u64 s = 0; s < nodes; s++) out_shared[s] = -1;
	std::vector<uint64_t> ca, cb;
	std::vector<SplitScored> sa, sb;
	NjTree t;
	u64 a0 = 0, n_shared = 0, n_scored = 0;
	for (u32 r0 = 0; r0 < rows;) {
		u32 r1 = r0;
		while (r1 < rows && (keys[r1] >> 20) == (keys[r0] >> 20)) r1++;
		const u32 m = r1 - r0;
		if (m > NJ_MAX_M) { vdjx_set_error("%s: clone %d has %u members (at most %u)", who, clone[row_item[r0]], m, NJ_MAX_M); return VDJX_ELIMIT; }
		u32 root[2] = {0, 0};                                 // a tree's root: the first member without a parent (a second one is refused below)
		const int32_t* par[2] = {parent_a, parent_b};
		for (int x = 0; x < 2; x++)
			for (u32 v = m; v-- > 0;)
				if (par[x][row_item[r0 + v]] < 0) root[x] = v;
		const u32 words = split_words(m);
		if (int rc = split_check(who, "the parents of tree a", parent_a, n, item_row.data(), row_item.data(), clone, r0, m, a0, root[0], lp, t)) return rc;
		if (m >= 4) { split_clades(m, t, ca); split_scored(m, root[0], t.root_kid, ca, sa); }
		if (int rc = split_check(who, "the parents of tree b", parent_b, n, item_row.data(), row_item.data(), clone, r0, m, a0, root[1], lp, t)) return rc;
		if (m >= 4) {
			split_clades(m, t, cb);
			split_scored(m, root[0], t.root_kid, cb, sb);      // (against tree a's root: the same side of every edge)
			for (const SplitScored& x : sa) {
				const uint64_t* mine = ca.data() + (size_t) (x.node - m) * words;
				int32_t hit = 0;
				for (const SplitScored& y : sb)
					if (y.sig == x.sig && std::equal(mine, mine + words, cb.data() + (size_t) (y.node - m) * words)) { hit = 1; break; }
				out_shared[n + a0 + (x.node - m)] = hit;
				n_shared += (u64) hit;
				n_scored++;
			}
		}
		if (m >= 3) a0 += m - 2;
		r0 = r1;
	}
	if (shared) *shared = n_shared;
	if (scored) *scored = n_scored;
	return VDJX_OK;
}
