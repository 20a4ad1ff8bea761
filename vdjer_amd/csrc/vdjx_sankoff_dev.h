// vdjx_sankoff_dev.h -- the device side that vdjx_tree_sankoff (vdjx_sankoff.hip) and vdjx_tree_sankoff_spr (vdjx_sankoff_spr.hip) share:
// the cost matrix as a kernel argument, the 16-byte messages and their 4 x 4 min-plus steps, the up pass and the down pass.  Moved here
// from vdjx_sankoff.hip as they were; the kernels have internal linkage, as vdjx_fitch.h's.
//
//   k_sk_up        one wave per (lineage, 64 columns), a lane per column: the messages in the host's post-order of the start tree, and W by
//                  one 64-bit integer atomicAdd per wave
//   k_sk_down      one wave per (lineage, 64 columns), parents before children in the host's order of the final tree: the states (a byte
//                  per inferred node and column), the ancestors' characters, and per edge its cost (64-bit) and mutations by one integer
//                  atomicAdd per (node, wave) of wave-reduced sums
#pragma once
#include "vdjx_common.h"
#include "vdjx_fitch.h"
#include "vdjx_treelay.h"

struct SkCost { u32 c[16]; };            // c[4 s + t], by value: kernel arguments
typedef unsigned long long ull;

__device__ inline u32 sk_code(char ch) { return ch == 'A' ? 0u : ch == 'C' ? 1u : ch == 'G' ? 2u : ch == 'T' ? 3u : 4u; }
__device__ inline uint4 sk_add(uint4 a, uint4 b) { return make_uint4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ inline bool sk_ne(uint4 a, uint4 b) { return a.x != b.x || a.y != b.y || a.z != b.z || a.w != b.w; }
// component i of a vector, i < 4
__device__ inline u32 sk_at(uint4 h, u32 i) { return i == 0 ? h.x : i == 1 ? h.y : i == 2 ? h.z : h.w; }
// the smallest component and the lowest index that has it
__device__ inline u32 sk_min(uint4 h) { return min(min(h.x, h.y), min(h.z, h.w)); }
__device__ inline u32 sk_argmin(uint4 h) {
	const u32 lo = sk_min(h);
	return h.x == lo ? 0u : h.y == lo ? 1u : h.z == lo ? 2u : 3u;
}
// row s of the matrix: c[s][0 .. 3]
__device__ inline uint4 sk_row(const SkCost& C, u32 s) {
	return make_uint4(s == 0 ? C.c[0] : s == 1 ? C.c[4] : s == 2 ? C.c[8] : C.c[12], s == 0 ? C.c[1] : s == 1 ? C.c[5] : s == 2 ? C.c[9] : C.c[13],
	                  s == 0 ? C.c[2] : s == 1 ? C.c[6] : s == 2 ? C.c[10] : C.c[14], s == 0 ? C.c[3] : s == 1 ? C.c[7] : s == 2 ? C.c[11] : C.c[15]);
}
// a leaf's message: column b of the matrix, 0 for a wildcard (b = 4)
__device__ inline uint4 sk_leaf_msg(const SkCost& C, u32 b) {
	if (b > 3u) return make_uint4(0u, 0u, 0u, 0u);
	return make_uint4(b == 0 ? C.c[0] : b == 1 ? C.c[1] : b == 2 ? C.c[2] : C.c[3], b == 0 ? C.c[4] : b == 1 ? C.c[5] : b == 2 ? C.c[6] : C.c[7],
	                  b == 0 ? C.c[8] : b == 1 ? C.c[9] : b == 2 ? C.c[10] : C.c[11], b == 0 ? C.c[12] : b == 1 ? C.c[13] : b == 2 ? C.c[14] : C.c[15]);
}
// an inferred node's message from its S: H(s) = min_t (c[s][t] + S[t])
__device__ inline uint4 sk_msg(const SkCost& C, uint4 S) {
	return make_uint4(min(min(C.c[0] + S.x, C.c[1] + S.y), min(C.c[2] + S.z, C.c[3] + S.w)), min(min(C.c[4] + S.x, C.c[5] + S.y), min(C.c[6] + S.z, C.c[7] + S.w)),
	                  min(min(C.c[8] + S.x, C.c[9] + S.y), min(C.c[10] + S.z, C.c[11] + S.w)), min(min(C.c[12] + S.x, C.c[13] + S.y), min(C.c[14] + S.z, C.c[15] + S.w)));
}
// a column's cost from the message of the root's child and the root's code
__device__ inline u32 sk_root_term(uint4 h, u32 rb) { return rb > 3u ? sk_min(h) : sk_at(h, rb); }

// NjFit describes the lineage as in vdjx_fitch.h; fs_off counts (inferred node, column) cells: the lineage's first message in msg_all and
// its first state in k_sk_down's bytes
static __global__ __launch_bounds__(64) void k_sk_up(const NjFitItem* __restrict__ items, const NjFit* __restrict__ fits, const char* __restrict__ contigs,
                                                     const TreeRow* __restrict__ ri, const u32* __restrict__ kid, const u32* __restrict__ order, uint4* msg_all,
                                                     ull* __restrict__ W, const SkCost C) {
	const NjFitItem it = items[blockIdx.x];
	const NjFit q = fits[it.lin];
	const u32 col = it.col0 + threadIdx.x, m = q.m;        // (m >= 2: the host makes no item for less)
	const bool live = col < q.w;
	const u32 cc = live ? col : 0u;
	uint4* H = msg_all + q.fs_off + cc;                    // + (v - m) * w
	const u32* ord = order + q.ord_off;
	auto code = [&](u32 y) { return sk_code(contigs[ri[q.first + y].at + cc]); };
	auto msg_of = [&](u32 y) { return y < m ? sk_leaf_msg(C, code(y)) : H[(size_t) (y - m) * q.w]; };
	for (u32 t = 0; t + 2u < m; t++) {
		const u32 v = ord[t];
		const uint4 h = sk_msg(C, sk_add(msg_of(kid[2u * (q.node0 + v - m)]), msg_of(kid[2u * (q.node0 + v - m) + 1u])));
		if (live) H[(size_t) (v - m) * q.w] = h;
	}
	const u64 sum = vdjx_wave_sum64(live ? (u64) sk_root_term(msg_of(q.root_kid), code(q.root)) : 0ull);
	if (threadIdx.x == 0 && sum) atomicAdd(W + it.lin, (ull) sum);
}

// one wave per item, a lane per window column.  order[]: the lineage's inferred nodes of the FINAL tree, children before parents; kid, par
// and leaf_par are the final tree's.  st_all: a byte per (inferred node, column).  cost_* / mut_*: zeroed by the host
static __global__ __launch_bounds__(64) void k_sk_down(const NjFitItem* __restrict__ items, const NjFit* __restrict__ fits, const char* __restrict__ contigs,
                                                       const TreeRow* __restrict__ ri, const u32* __restrict__ kid, const u32* __restrict__ par,
                                                       const u32* __restrict__ order, const u32* __restrict__ leaf_par, const uint4* __restrict__ msg_all,
                                                       uint8_t* st_all, ull* cost_row, ull* cost_inf, u32* mut_row, u32* mut_inf, char* __restrict__ anc, u32 len,
                                                       const SkCost C) {
	const NjFitItem it = items[blockIdx.x];
	const NjFit q = fits[it.lin];
	const u32 col = it.col0 + threadIdx.x, m = q.m, inner = m - 2u;      // (m >= 2)
	const bool live = col < q.w;
	const u32 cc = live ? col : 0u;
	const uint4* H = msg_all + q.fs_off + cc;
	uint8_t* st = st_all + q.fs_off + cc;
	const u32* ord = order + q.ord_off;
	auto code = [&](u32 y) { return sk_code(contigs[ri[q.first + y].at + cc]); };
	auto msg_of = [&](u32 y) { return y < m ? sk_leaf_msg(C, code(y)) : H[(size_t) (y - m) * q.w]; };
	const u32 rb = code(q.root);
	const u32 rstate = rb > 3u ? sk_argmin(msg_of(q.root_kid)) : rb;
	auto edge = [&](u32 ps, u32 state, ull* cost_at, u32* mut_at) {
		const u64 paid = vdjx_wave_sum64(live ? (u64) sk_at(sk_row(C, ps), state) : 0ull);
		const u64 diff = __ballot(live && state != ps);
		if (threadIdx.x == 0 && paid) atomicAdd(cost_at, (ull) paid);
		if (threadIdx.x == 0 && diff) atomicAdd(mut_at, (u32) __popcll(diff));
	};
	for (u32 t = m > 2u ? inner : 0u; t-- > 0u;) {         // parents before children
		const u32 v = ord[t], p = par[q.node0 + v - m];
		const u32 ps = p == q.root ? rstate : (u32) st[(size_t) (p - m) * q.w];
		const uint4 S = sk_add(msg_of(kid[2u * (q.node0 + v - m)]), msg_of(kid[2u * (q.node0 + v - m) + 1u]));
		const u32 state = sk_argmin(sk_add(sk_row(C, ps), S));
		if (live) {
			st[(size_t) (v - m) * q.w] = (uint8_t) state;
			if (anc) anc[(size_t) (q.node0 + v - m) * len + col] = "ACGT"[state];
		}
		edge(ps, state, cost_inf + q.node0 + v - m, mut_inf + q.node0 + v - m);
	}
	for (u32 y = 0; y < m; y++) {
		if (y == q.root) continue;
		const u32 up = leaf_par[q.first + y];
		const u32 ps = up == q.root ? rstate : (u32) st[(size_t) (up - m) * q.w], b = code(y);
		edge(ps, b > 3u ? ps : b, cost_row + q.first + y, mut_row + q.first + y);
	}
}
