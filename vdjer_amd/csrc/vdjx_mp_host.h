// vdjx_mp_host.h -- the host side of vdjx_tree_mp (vdjx_mp.hip): a lineage's tree from its nodes' parents.  Plain C++, no GPU:
// profiles/mp_host_check.cpp runs it under a sanitizer, on parents no device run would give as well.
//
//   mp_local         an output slot as a local node id of one lineage (leaves 0 .. m - 1, inferred nodes m .. 2m - 3), or MP_OUTSIDE
//   mp_orient        the local parents of one lineage's nodes, rooted at leaf `root` (whose own entry is not read): depth of every node,
//                    the two children of every inferred node (ascending), the root's child and the inferred nodes in post-order
//                    (children before parents) in an NjTree.  O(nodes).  It is both the check of a caller's start tree and, after the
//                    search, what turns the device's final kid / par into Fitch's input.  MP_OK, or what is wrong with the parents
// Everything here has internal linkage.
#pragma once
#include "vdjx_nj_host.h"

#define MP_OUTSIDE (-2)

enum { MP_OK = 0, MP_BAD_ARG, MP_PARENT_OUTSIDE, MP_ROOT_KIDS, MP_INFERRED_KIDS, MP_LEAF_KIDS, MP_CYCLE };

namespace {

inline const char* mp_why(int e) {
	switch (e) {
		case MP_PARENT_OUTSIDE: return "a node's parent is outside the lineage";
		case MP_ROOT_KIDS: return "the root leaf has not exactly one child";
		case MP_INFERRED_KIDS: return "an inferred node has not exactly two children";
		case MP_LEAF_KIDS: return "a leaf other than the root has children";
		case MP_CYCLE: return "the parents hold a cycle";
		default: return "bad arguments";
	}
}

// slot: an entry of start_parent.  item_row[i]: the row of item i (-1: in no lineage).  The lineage: rows [first, first + m), its inferred
// nodes the slots n + a0 .. n + a0 + m - 3
inline int32_t mp_local(int64_t slot, size_t n, const int32_t* item_row, uint32_t first, uint32_t m, uint64_t a0) {
	if (slot < 0) return MP_OUTSIDE;
	if ((uint64_t) slot < n) {
		const int32_t r = item_row[slot];
		return r >= (int32_t) first && (uint32_t) r < first + m ? r - (int32_t) first : MP_OUTSIDE;
	}
	const uint64_t a = (uint64_t) slot - n;
	return m > 2 && a >= a0 && a < a0 + (m - 2) ? (int32_t) (m + (a - a0)) : MP_OUTSIDE;
}

inline int mp_orient(uint32_t m, uint32_t root, const int32_t* parent, NjTree& t) {
	if (m == 0 || m > NJ_MAX_M || root >= m) return MP_BAD_ARG;
	const uint32_t nodes = m < 3 ? m : 2 * m - 2;
	t.parent.assign(nodes, -1);
	t.depth.assign(nodes, -1);
	t.length.assign(nodes, 0);
	t.kid.assign(2 * (size_t) (nodes - m), 0);
	t.order.clear();
	t.root_kid = 0;
	std::vector<uint8_t> kids(nodes, 0);
	for (uint32_t v = 0; v < nodes; v++) {
		if (v == root) continue;
		const int32_t p = parent[v];
		if (p < 0 || (uint32_t) p >= nodes) return MP_PARENT_OUTSIDE;
		t.parent[v] = p;
		if ((uint32_t) p == root) {
			if (kids[p]++) return MP_ROOT_KIDS;
			t.root_kid = v;
		} else if ((uint32_t) p < m) return MP_LEAF_KIDS;
		else {
			if (kids[p] == 2) return MP_INFERRED_KIDS;
			t.kid[2 * (size_t) (p - m) + kids[p]++] = v;      // (v ascends: so do a node's children)
		}
	}
	if (m >= 2 && kids[root] != 1) return MP_ROOT_KIDS;
	for (uint32_t v = m; v < nodes; v++)
		if (kids[v] != 2) return MP_INFERRED_KIDS;
	// depth first from the root: every node has the children it should have, so whatever is not reached hangs in a cycle
	std::vector<uint32_t> stack;
	std::vector<uint8_t> seen(nodes, 0);
	t.depth[root] = 0;
	uint32_t reached = 1;
	if (m >= 2) stack.push_back(t.root_kid);
	while (!stack.empty()) {
		const uint32_t v = stack.back();
		if (seen[v]) {
			stack.pop_back();
			if (v >= m) t.order.push_back(v);
			continue;
		}
		seen[v] = 1;
		reached++;
		t.depth[v] = t.depth[t.parent[v]] + 1;
		if (v < m) continue;                                 // (popped at its second visit)
		stack.push_back(t.kid[2 * (size_t) (v - m)]);
		stack.push_back(t.kid[2 * (size_t) (v - m) + 1]);
	}
	return reached == nodes ? MP_OK : MP_CYCLE;
}

}  // namespace
