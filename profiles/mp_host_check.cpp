// mp_host_check.cpp -- the host side of vdjx_tree_mp (vdjer_amd/csrc/vdjx_mp_host.h: slots to local ids, the check of a start tree and the
// rooting of the final parents) on the CPU, stand-alone, for a run under a sanitizer:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I vdjer_amd/csrc profiles/mp_host_check.cpp -o mp_host_check && ./mp_host_check
// Random binary trees of 1 .. 300 leaves rooted at a random leaf, given as parents: each result is checked against a plain recount, and
// against nj_orient on the same tree's edges.  Then random nearest-neighbour interchanges, as the device applies them, must keep the
// parents a tree.  Then parents no device run gives -- every kind the start check names, ids out of range, m = 0 and m past the limit --
// all must be refused, none may touch memory it does not own.  Prints "ok" and returns 0.
#include "vdjx_mp_host.h"

#include <stdio.h>

#include <random>

static int fail(const char* what, size_t m) {
	fprintf(stderr, "mp_host_check: %s (m = %zu)\n", what, m);
	return 1;
}

// leaves 0 .. m - 1, inner nodes m .. 2m - 3: every new leaf into a random edge, then rooted at `root` through nj_orient
static bool random_parents(uint32_t m, uint32_t root, std::mt19937& rng, std::vector<int32_t>& parent, NjTree& t) {
	std::vector<uint32_t> a, b;
	auto add = [&](uint32_t x, uint32_t y) { a.push_back(x); b.push_back(y); };
	if (m == 2) add(0, 1);
	if (m >= 3) {
		add(0, m); add(1, m); add(2, m);
		uint32_t next = m + 1;
		for (uint32_t leaf = 3; leaf < m; leaf++) {
			const size_t k = rng() % a.size();
			const uint32_t y = b[k];
			b[k] = next;
			add(next, y);
			add(leaf, next);
			next++;
		}
	}
	std::vector<int64_t> len(a.size() + 1, 0);
	if (!nj_orient(m, a.data(), b.data(), len.data(), root, t)) return false;
	parent = t.parent;
	return true;
}

static int check_tree(uint32_t m, const std::vector<int32_t>& parent, uint32_t root, const NjTree* same) {
	const uint32_t nodes = m < 3 ? m : 2 * m - 2;
	NjTree t;
	if (mp_orient(m, root, parent.data(), t) != MP_OK) return fail("a tree was refused", m);
	if (t.parent.size() != nodes || t.depth.size() != nodes || t.order.size() != nodes - m || t.kid.size() != 2 * (size_t) (nodes - m)) return fail("sizes", m);
	std::vector<uint32_t> kids(nodes, 0), seen(nodes, 0);
	for (uint32_t v = 0; v < nodes; v++) {
		if ((t.parent[v] < 0) != (v == root)) return fail("root", m);
		if (v == root) { if (t.depth[v] != 0) return fail("root depth", m); continue; }
		if (t.parent[v] != parent[v] || t.depth[v] != t.depth[t.parent[v]] + 1) return fail("depth", m);
		kids[t.parent[v]]++;
	}
	for (uint32_t v = 0; v < nodes; v++)
		if (kids[v] != (v >= m ? 2u : (v == root && m >= 2 ? 1u : 0u))) return fail("children", m);
	for (uint32_t v : t.order) {                           // children before parents
		if (v < m || seen[v]) return fail("order", m);
		for (int k = 0; k < 2; k++) {
			const uint32_t c = t.kid[2 * (size_t) (v - m) + k];
			if (t.parent[c] != (int32_t) v || (c >= m && !seen[c])) return fail("order of children", m);
		}
		if (t.kid[2 * (size_t) (v - m)] >= t.kid[2 * (size_t) (v - m) + 1]) return fail("children ascend", m);
		seen[v] = 1;
	}
	if (m >= 2 && t.parent[t.root_kid] != (int32_t) root) return fail("root_kid", m);
	if (same && (same->depth != t.depth || same->kid != t.kid || same->root_kid != t.root_kid)) return fail("not nj_orient's tree", m);
	return 0;
}

// the candidate (v, k) as k_mp_pick rewires it, on parents alone
static void interchange(uint32_t m, std::vector<int32_t>& parent, const NjTree& t, uint32_t v, uint32_t k) {
	const uint32_t p = (uint32_t) parent[v];
	const uint32_t s = t.kid[2 * (size_t) (p - m)] == v ? t.kid[2 * (size_t) (p - m) + 1] : t.kid[2 * (size_t) (p - m)], c = t.kid[2 * (size_t) (v - m) + k];
	parent[s] = (int32_t) v;
	parent[c] = (int32_t) p;
}

static int refused(uint32_t m, uint32_t root, const std::vector<int32_t>& parent, int want, const char* what) {
	NjTree t;
	const int e = mp_orient(m, root, parent.data(), t);
	if (e == MP_OK || (want && e != want)) return fail(what, m);
	if (!mp_why(e) || !mp_why(e)[0]) return fail("no reason", m);
	return 0;
}

int main() {
	std::mt19937 rng(2026);
	for (uint32_t m = 1; m <= 300; m += m < 12 ? 1 : 17)
		for (int round = 0; round < 8; round++) {
			const uint32_t root = rng() % m;
			std::vector<int32_t> parent;
			NjTree t;
			if (!random_parents(m, root, rng, parent, t)) return fail("the generator", m);
			if (check_tree(m, parent, root, &t)) return 1;
			for (int move = 0; m > 3 && move < 20; move++) {
				std::vector<uint32_t> cand;
				for (uint32_t v = m; v < 2 * m - 2; v++)
					if ((uint32_t) parent[v] >= m) cand.push_back(v);
				if (cand.size() != m - 3) return fail("candidates", m);
				interchange(m, parent, t, cand[rng() % cand.size()], rng() % 2);
				if (check_tree(m, parent, root, nullptr)) return 1;
				if (mp_orient(m, root, parent.data(), t) != MP_OK) return fail("after a move", m);
			}
		}
	// m = 5, root 0: leaves 1 .. 4, inferred 5, 6, 7; the caterpillar 0 <- 5 <- {1, 6}, 6 <- {2, 7}, 7 <- {3, 4}
	const std::vector<int32_t> good = {-1, 5, 6, 7, 7, 0, 5, 6};
	if (check_tree(5, good, 0, nullptr)) return 1;
	auto with = [&](size_t v, int32_t p) { std::vector<int32_t> x = good; x[v] = p; return x; };
	if (refused(5, 0, with(1, MP_OUTSIDE), MP_PARENT_OUTSIDE, "a parent outside the lineage was accepted")) return 1;
	if (refused(5, 0, with(1, -1), MP_PARENT_OUTSIDE, "a second root was accepted")) return 1;
	if (refused(5, 0, with(1, 8), MP_PARENT_OUTSIDE, "a parent past the last node was accepted")) return 1;
	if (refused(5, 0, with(1, 0), MP_ROOT_KIDS, "a root leaf with two children was accepted")) return 1;
	if (refused(5, 0, with(5, 6), 0, "a root leaf without a child was accepted")) return 1;
	if (refused(5, 0, with(4, 5), MP_INFERRED_KIDS, "an inferred node with three children was accepted")) return 1;
	if (refused(5, 0, with(4, 1), MP_LEAF_KIDS, "a leaf with children was accepted")) return 1;
	if (refused(5, 0, with(4, 4), MP_LEAF_KIDS, "a leaf that is its own parent was accepted")) return 1;
	if (refused(5, 0, {-1, 5, 5, 6, 7, 0, 7, 6}, MP_CYCLE, "a cycle was accepted")) return 1;
	if (refused(5, 0, {-1, 5, 5, 6, 6, 0, 7, 7}, 0, "an inferred node that is its own parent was accepted")) return 1;
	if (refused(5, 5, good, MP_BAD_ARG, "a root that is no leaf was accepted")) return 1;
	if (refused(0, 0, {}, MP_BAD_ARG, "m = 0 was accepted") || refused(NJ_MAX_M + 1, 0, {}, MP_BAD_ARG, "m past the limit was accepted")) return 1;
	if (refused(2, 0, {-1, 1}, MP_LEAF_KIDS, "a loop on the one edge was accepted")) return 1;
	if (check_tree(2, {5, 0}, 0, nullptr) || check_tree(1, {9}, 0, nullptr)) return 1;      // (the root's own entry is not read)
	// slots to local ids: items 0 .. 5, rows of the lineage 2 .. 4 (items 4, 1, 5), its inferred nodes the call's 3rd on
	const int32_t item_row[6] = {0, 3, -1, 1, 2, 4};
	const struct { int64_t slot; int32_t want; } map[] = {{4, 0}, {1, 1}, {5, 2}, {0, MP_OUTSIDE}, {2, MP_OUTSIDE}, {3, MP_OUTSIDE}, {-1, MP_OUTSIDE},
	                                                      {6 + 3, 3}, {6 + 2, MP_OUTSIDE}, {6 + 4, MP_OUTSIDE}, {1ll << 40, MP_OUTSIDE}};
	for (const auto& q : map)
		if (mp_local(q.slot, 6, item_row, 2, 3, 3) != q.want) return fail("slot to local id", (size_t) q.slot);
	if (mp_local(6, 6, item_row, 0, 2, 0) != MP_OUTSIDE) return fail("an inferred node of a lineage of two", 2);
	puts("ok");
	return 0;
}
