// vdjx_nj_host.h -- the host side of vdjx_tree_nj (vdjx_nj.hip): counting the nodes, and turning a lineage's joined edges into a rooted
// tree.  Plain C++, no GPU: profiles/nj_host_check.cpp runs it under a sanitizer, on edge lists no device run would give as well.
//
//   nj_count_nodes   n + the sum of max(0, m - 2) over the clones: the slots of vdjx_tree_nj's outputs
//   nj_orient        the 2m - 3 edges (a, b, length) of one lineage -- leaves 0 .. m - 1, inferred nodes m .. 2m - 3 -- rooted at a leaf:
//                    parent, length and depth of every node, the two children of every inferred node (ascending) and the inferred nodes
//                    in post-order (children before parents).  O(nodes); false where the edges are not such a tree
// The batches are vdjx_link.h's link_batches.  Everything here has internal linkage.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#define NJ_MAX_M 4096u                   // members of a lineage

struct NjTree {
	std::vector<int32_t> parent, depth;                   // per node of the lineage (local ids); the root's parent is -1
	std::vector<int64_t> length;                          // of the edge to the parent; 0 for the root
	std::vector<uint32_t> kid;                            // [2 * (v - m)], [2 * (v - m) + 1]: the children of inferred node v, ascending
	std::vector<uint32_t> order;                          // the inferred nodes, children before parents
	uint32_t root_kid = 0;                                // the root leaf's one child (m >= 2)
};

namespace {

// false: a clone below -1
inline bool nj_count_nodes(const int32_t* clone, size_t n, uint64_t* nodes) {
	std::vector<int32_t> keys;
	for (size_t i = 0; i < n; i++) {
		if (clone[i] < -1) return false;
		if (clone[i] >= 0) keys.push_back(clone[i]);
	}
	std::sort(keys.begin(), keys.end());
	uint64_t total = n;
	for (size_t a = 0; a < keys.size();) {
		size_t b = a;
		while (b < keys.size() && keys[b] == keys[a]) b++;
		if (b - a > 2) total += b - a - 2;
		a = b;
	}
	*nodes = total;
	return true;
}

inline bool nj_orient(uint32_t m, const uint32_t* ea, const uint32_t* eb, const int64_t* elen, uint32_t root, NjTree& t) {
	if (m == 0 || m > NJ_MAX_M || root >= m) return false;
	const uint32_t nodes = m < 3 ? m : 2 * m - 2, ne = m < 2 ? 0 : 2 * m - 3;
	t.parent.assign(nodes, -1);
	t.depth.assign(nodes, -1);
	t.length.assign(nodes, 0);
	t.kid.assign(2 * (size_t) (nodes - m), 0);
	t.order.clear();
	t.root_kid = 0;
	std::vector<uint32_t> deg(nodes + 1, 0);
	for (uint32_t e = 0; e < ne; e++) {
		if (ea[e] >= nodes || eb[e] >= nodes || ea[e] == eb[e]) return false;
		deg[ea[e] + 1]++;
		deg[eb[e] + 1]++;
	}
	for (uint32_t v = 0; v < nodes; v++) {
		if (m >= 2 && deg[v + 1] != (v < m ? 1u : 3u)) return false;      // a leaf has one neighbour, an inferred node three
		deg[v + 1] += deg[v];
	}
	std::vector<uint32_t> fill(deg.begin(), deg.end() - 1), adj(2 * (size_t) ne), adj_e(2 * (size_t) ne);
	for (uint32_t e = 0; e < ne; e++) {
		adj[fill[ea[e]]] = eb[e]; adj_e[fill[ea[e]]++] = e;
		adj[fill[eb[e]]] = ea[e]; adj_e[fill[eb[e]]++] = e;
	}
	// depth first from the root: a node is pushed when it is reached and emitted (inferred nodes only) when it is popped the second time
	std::vector<uint32_t> stack;
	std::vector<uint8_t> seen(nodes, 0);
	t.depth[root] = 0;
	stack.push_back(root);
	uint32_t reached = 1;
	while (!stack.empty()) {
		const uint32_t v = stack.back();
		if (seen[v]) {
			stack.pop_back();
			if (v >= m) t.order.push_back(v);
			continue;
		}
		seen[v] = 1;
		uint32_t kids = 0, k2[2] = {0, 0};
		for (uint32_t k = deg[v]; k < deg[v + 1]; k++) {
			const uint32_t c = adj[k];
			if (t.depth[c] >= 0) continue;                    // (its parent: the only neighbour reached before -- or a cycle, caught by the count)
			t.parent[c] = (int32_t) v;
			t.length[c] = elen[adj_e[k]];
			t.depth[c] = t.depth[v] + 1;
			reached++;
			if (kids < 2) k2[kids] = c;
			kids++;
			stack.push_back(c);
		}
		if (v >= m) {
			if (kids != 2) return false;
			t.kid[2 * (size_t) (v - m)] = std::min(k2[0], k2[1]);
			t.kid[2 * (size_t) (v - m) + 1] = std::max(k2[0], k2[1]);
		} else if (v == root) {
			if (kids != (m >= 2 ? 1u : 0u)) return false;
			t.root_kid = k2[0];
		} else if (kids) return false;
	}
	return reached == nodes && t.order.size() == nodes - m;
}

}  // namespace
