// vdjx_unionfind.h -- the lock-free union-find vdjx_lineage.hip and vdjx_tree.hip share (gfx950 only).
//
// parent[] over item indices: find with path halving (atomicMin: a parent only ever gets smaller), union by atomicCAS on the LARGER root,
// which is hooked under the smaller.  parent[x] <= x always holds, so the trees stay trees and the root of a finished component is its
// smallest member whatever the interleaving was.
#pragma once
#include "vdjx_common.h"

// a word another wave may be changing: read past this CU's L1
__device__ inline u32 uf_peek(const u32* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ inline u32 uf_find(u32* parent, u32 x) {
	for (;;) {
		const u32 p = uf_peek(parent + x);
		if (p == x) return x;
		const u32 g = uf_peek(parent + p);
		if (g != p) atomicMin(parent + x, g);          // (path halving; g is an ancestor of x and smaller than p)
		x = g;
	}
}

__device__ inline void uf_unite(u32* parent, u32 a, u32 b) {
	for (;;) {
		a = uf_find(parent, a);
		b = uf_find(parent, b);
		if (a == b) return;
		const u32 hi = a > b ? a : b, lo = a > b ? b : a;
		const u32 old = atomicCAS(parent + hi, hi, lo);
		if (old == hi) return;                          // hooked (lo may have stopped being a root meanwhile: it is a member all the same)
		a = old;                                        // somebody else hooked hi first: go on from where it hangs now
		b = lo;
	}
}
