// vdjx_fitch.h -- Fitch parsimony on a rooted lineage tree, a lane per window column: what vdjx_nj.hip, vdjx_mp.hip and vdjx_spr.hip share
// (gfx950 only, wave64).  k_nj_fitch moved here from vdjx_nj.hip as it was, k_mp_up (below) from vdjx_mp.hip; `static` because several
// translation units include them.
//   k_nj_fitch     one wave per (lineage, 64 window columns), a lane per column: the column is the fastest index of everything it touches.
//                  The up-pass walks the inferred nodes in post-order and writes one set per (node, column) -- a byte -- into workspace;
//                  the down-pass walks them back, overwrites the set with the state, writes the ancestor's character and counts the lanes
//                  whose state differs from the parent's: one integer atomicAdd per (node, wave).  The leaves follow.
#pragma once
#include "vdjx_common.h"
#include "vdjx_treelay.h"

// Fitch: a lineage's rooted tree as the host laid it out.  Nodes are local ids (leaves 0 .. m - 1 = rows first .. first + m - 1, inferred
// nodes from m on); inferred node v has index node0 + v - m in kid[][2], par[], and in the call's inferred slots (mutations, ancestors)
struct NjFit { u64 fs_off; u32 first, m, w, node0, root, root_kid, ord_off, pad; };
static_assert(sizeof(NjFit) == 40, "uploaded as it is");
struct NjFitItem { u32 lin, col0; };

__device__ inline u32 nj_leaf_set(char ch) { return ch == 'A' ? 1u : ch == 'C' ? 2u : ch == 'G' ? 4u : ch == 'T' ? 8u : 15u; }
__device__ inline u32 nj_lowest(u32 s) { return (u32) __ffs((int) s) - 1u; }
// Fitch's rule for two children's sets and its union event: vdjx_mp.hip and vdjx_spr.hip score with them (moved here from vdjx_mp.hip as they were)
__device__ inline u32 mp_comb(u32 a, u32 b) { return (a & b) ? (a & b) : (a | b); }
__device__ inline int mp_flag(u32 a, u32 b) { return (a & b) ? 0 : 1; }

// one wave per item, a lane per window column.  fs: a byte per (inferred node, column), first the set, then the state.  order[]: the
// lineage's inferred nodes, children before parents.  leaf_par[row]: a leaf's parent (local id).  mut_row / mut_inf: zeroed by the host.
static __global__ __launch_bounds__(64) void k_nj_fitch(const NjFitItem* __restrict__ items, const NjFit* __restrict__ fits, const char* __restrict__ contigs,
                                                 const TreeRow* __restrict__ ri, const u32* __restrict__ kid, const u32* __restrict__ par,
                                                 const u32* __restrict__ order, const u32* __restrict__ leaf_par, uint8_t* __restrict__ fs_all,
                                                 u32* mut_row, u32* mut_inf, char* __restrict__ anc, u32 len) {
	const NjFitItem it = items[blockIdx.x];
	const NjFit q = fits[it.lin];
	const u32 col = it.col0 + threadIdx.x, m = q.m, inner = m - 2u;      // (m >= 2: the host makes no item for less)
	const bool live = col < q.w;
	const u32 cc = live ? col : 0u;
	uint8_t* fs = fs_all + q.fs_off + cc;                  // + (v - m) * w
	const u32* ord = order + q.ord_off;
	auto leaf = [&](u32 p) { return nj_leaf_set(contigs[ri[q.first + p].at + cc]); };
	auto set_of = [&](u32 v) { return v < m ? leaf(v) : (u32) fs[(size_t) (v - m) * q.w]; };
	for (u32 t = 0; t < (m > 2u ? inner : 0u); t++) {
		const u32 v = ord[t], a = set_of(kid[2u * (q.node0 + v - m)]), b = set_of(kid[2u * (q.node0 + v - m) + 1u]);
		if (live) fs[(size_t) (v - m) * q.w] = (uint8_t) ((a & b) ? (a & b) : (a | b));
	}
	const u32 rs = leaf(q.root), cs = set_of(q.root_kid);
	const u32 rstate = nj_lowest((rs & cs) ? (rs & cs) : rs);
	for (u32 t = m > 2u ? inner : 0u; t-- > 0u;) {         // parents before children
		const u32 v = ord[t], p = par[q.node0 + v - m];
		const u32 ps = p == q.root ? rstate : (u32) fs[(size_t) (p - m) * q.w], s = fs[(size_t) (v - m) * q.w];
		const u32 st = (s >> ps & 1u) ? ps : nj_lowest(s);
		if (live) {
			fs[(size_t) (v - m) * q.w] = (uint8_t) st;
			if (anc) anc[(size_t) (q.node0 + v - m) * len + col] = "ACGT"[st];
		}
		const u64 diff = __ballot(live && st != ps);
		if (threadIdx.x == 0 && diff) atomicAdd(mut_inf + q.node0 + v - m, (u32) __popcll(diff));
	}
	for (u32 p = 0; p < m; p++) {
		if (p == q.root) continue;
		const u32 up = leaf_par[q.first + p];
		const u32 ps = up == q.root ? rstate : (u32) fs[(size_t) (up - m) * q.w], s = leaf(p);
		const u32 st = (s >> ps & 1u) ? ps : nj_lowest(s);
		const u64 diff = __ballot(live && st != ps);
		if (threadIdx.x == 0 && diff) atomicAdd(mut_row + q.first + p, (u32) __popcll(diff));
	}
}

// the up sets of a start tree and its P: one wave per (lineage, 64 columns), a lane per column, the sets in the host's post-order, P by one
// integer atomicAdd per wave of the ballots' popcounts.  NjFit describes the lineage: fs_off its first set, node0 its first inferred node
// among the batch's, ord_off its post-order.  Moved here from vdjx_mp.hip as it was; `static` because vdjx_mp.hip and vdjx_spr.hip include it
static __global__ __launch_bounds__(64) void k_mp_up(const NjFitItem* __restrict__ items, const NjFit* __restrict__ fits, const char* __restrict__ contigs,
                                              const TreeRow* __restrict__ ri, const u32* __restrict__ kid, const u32* __restrict__ order,
                                              uint8_t* __restrict__ up_all, u32* __restrict__ P) {
	const NjFitItem it = items[blockIdx.x];
	const NjFit q = fits[it.lin];
	const u32 col = it.col0 + threadIdx.x, m = q.m;        // (m >= 2: the host makes no item for less)
	const bool live = col < q.w;
	const u32 cc = live ? col : 0u;
	uint8_t* up = up_all + q.fs_off + cc;                  // + (v - m) * w
	const u32* ord = order + q.ord_off;
	auto leaf = [&](u32 p) { return nj_leaf_set(contigs[ri[q.first + p].at + cc]); };
	auto set_of = [&](u32 v) { return v < m ? leaf(v) : (u32) up[(size_t) (v - m) * q.w]; };
	u32 events = 0;
	for (u32 t = 0; t + 2u < m; t++) {
		const u32 v = ord[t], a = set_of(kid[2u * (q.node0 + v - m)]), b = set_of(kid[2u * (q.node0 + v - m) + 1u]);
		if (live) up[(size_t) (v - m) * q.w] = (uint8_t) mp_comb(a, b);
		events += (u32) __popcll(__ballot(live && !(a & b)));
	}
	events += (u32) __popcll(__ballot(live && !(leaf(q.root) & set_of(q.root_kid))));
	if (threadIdx.x == 0 && events) atomicAdd(P + it.lin, events);
}
