// vdjx_spr_host.h -- the host side of vdjx_tree_spr (vdjx_spr.hip) that is no kernel launch: subtree pruning and regrafting on a lineage's
// local parents.  Plain C++, no GPU: profiles/spr_host_check.cpp runs it under a sanitizer.
//
//   spr_candidates   the candidates (c, y) of one scoring round of a rooted tree (an NjTree of mp_orient): the sum over the pruned nodes c
//                    -- every node but the root leaf and its child -- of 2 (m - leaves(c)) - 4.  vdjx_tree_spr checks the device's count
//                    of a lineage's first round against it
//   spr_legal        whether (c, y) is a candidate of the tree the parents describe
//   spr_apply        the move on the parents (include/vdjx.h, "apply"): with p = parent(c), s p's other child and g = parent(p), s hangs
//                    under g, p under y's parent and y under p.  Children lists are not kept here: mp_orient sorts them.  The inverse of
//                    (c, y) is (c, s).  The device rewires kid / par by the same rule (k_spr_pick); this is its statement on the host, and
//                    what the check program holds mp_orient and spr_candidates against
// Everything here has internal linkage.
#pragma once
#include "vdjx_mp_host.h"

namespace {

inline uint64_t spr_candidates(uint32_t m, uint32_t root, const NjTree& t) {
	if (m < 4) return 0;
	std::vector<uint32_t> leaves(2 * (size_t) m - 2, 1u);
	for (uint32_t v : t.order) leaves[v] = leaves[t.kid[2 * (size_t) (v - m)]] + leaves[t.kid[2 * (size_t) (v - m) + 1]];   // children first
	uint64_t sum = 0;
	for (uint32_t c = 0; c < 2 * m - 2; c++)
		if (c != root && c != t.root_kid) sum += 2ull * (m - leaves[c]) - 4;
	return sum;
}

// the other child of p (local parents; the root's own entry is not read)
inline int32_t spr_sibling(uint32_t nodes, uint32_t root, const int32_t* parent, uint32_t p, uint32_t c) {
	for (uint32_t v = 0; v < nodes; v++)
		if (v != root && v != c && parent[v] == (int32_t) p) return (int32_t) v;
	return -1;
}

inline bool spr_legal(uint32_t m, uint32_t root, const int32_t* parent, uint32_t c, uint32_t y) {
	const uint32_t nodes = 2 * m - 2;
	if (m < 4 || c >= nodes || y >= nodes || c == root || y == root || parent[c] == (int32_t) root) return false;
	const uint32_t p = (uint32_t) parent[c];
	if (y == p || (int32_t) y == spr_sibling(nodes, root, parent, p, c)) return false;
	for (uint32_t v = y; v != root; v = (uint32_t) parent[v])          // y inside c's subtree
		if (v == c) return false;
	return true;
}

// applies a legal (c, y); returns s, so that (c, s) undoes it
inline uint32_t spr_apply(uint32_t m, uint32_t root, int32_t* parent, uint32_t c, uint32_t y) {
	const uint32_t p = (uint32_t) parent[c], s = (uint32_t) spr_sibling(2 * m - 2, root, parent, p, c);
	parent[s] = parent[p];
	parent[p] = parent[y];
	parent[y] = (int32_t) p;
	return s;
}

}  // namespace
