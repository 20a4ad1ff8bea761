// nj_host_check.cpp -- the host side of vdjx_tree_nj (vdjer_amd/csrc/vdjx_nj_host.h: node count, rooting and post-order; vdjx_link.h: the
// batches; vdjer_amd/csrc/host/vdjx_newick.h: the Newick writer) on the CPU, stand-alone, for a run under a sanitizer:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I vdjer_amd/csrc -I vdjer_amd/csrc/host profiles/nj_host_check.cpp -o nj_host_check && ./nj_host_check
// Random binary trees of 1 .. 300 leaves (every new leaf into a random edge), rooted at every kind of leaf: each result is checked against
// a plain recount, and the Newick text is parsed back.  Then edge lists no device run gives: ids out of range, self loops, a doubled edge
// (a cycle beside a loose node), a star, a root that is no leaf, m = 0 and m past the limit -- all must be refused, none may touch memory
// it does not own.  Prints "ok" and returns 0.
#include "vdjx_link.h"
#include "vdjx_nj_host.h"
#include "vdjx_newick.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <random>
#include <string>

static int fail(const char* what, size_t m) {
	fprintf(stderr, "nj_host_check: %s (m = %zu)\n", what, m);
	return 1;
}

struct Edges { std::vector<uint32_t> a, b; std::vector<int64_t> len; };

// leaves 0 .. m - 1, inner nodes m .. 2m - 3, in any creation order (nj_orient does not depend on it)
static Edges random_tree(uint32_t m, std::mt19937& rng) {
	Edges e;
	auto add = [&](uint32_t x, uint32_t y) { e.a.push_back(x); e.b.push_back(y); e.len.push_back((int64_t) (rng() % 7) * 65536 - 65536); };
	if (m == 2) add(0, 1);
	if (m < 3) return e;
	add(0, m); add(1, m); add(2, m);
	uint32_t next = m + 1;
	for (uint32_t leaf = 3; leaf < m; leaf++) {
		const size_t k = rng() % e.a.size();
		const uint32_t y = e.b[k];
		e.b[k] = next;                                      // a -- next, next -- y, leaf -- next
		add(next, y);
		add(leaf, next);
		next++;
	}
	return e;
}

static void label(FILE* fp, size_t s, void*) { fprintf(fp, "n%zu", s); }

static int check_tree(uint32_t m, std::mt19937& rng) {
	const Edges e = random_tree(m, rng);
	const uint32_t nodes = m < 3 ? m : 2 * m - 2, root = rng() % m;
	NjTree t;
	if (!nj_orient(m, e.a.data(), e.b.data(), e.len.data(), root, t)) return fail("a tree was refused", m);
	if (t.parent.size() != nodes || t.order.size() != nodes - m) return fail("sizes", m);
	int64_t total = 0, want = 0;
	for (int64_t x : e.len) want += x;
	std::vector<uint32_t> kids(nodes, 0), seen(nodes, 0);
	for (uint32_t v = 0; v < nodes; v++) {
		if ((t.parent[v] < 0) != (v == root)) return fail("root", m);
		if (v == root) { if (t.depth[v] != 0 || t.length[v] != 0) return fail("root fields", m); continue; }
		if (t.depth[v] != t.depth[t.parent[v]] + 1) return fail("depth", m);
		kids[t.parent[v]]++;
		total += t.length[v];
	}
	if (total != want) return fail("lengths", m);
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
	// the Newick text: as many labels as nodes, balanced, every child list in ascending slot
	std::vector<size_t> kid_off(nodes + 1);
	std::vector<uint32_t> kid(nodes);
	if (newick_children(t.parent.data(), nodes, kid_off.data(), kid.data())) return fail("children of a tree refused", m);
	char* text = nullptr;
	size_t bytes = 0;
	FILE* fp = open_memstream(&text, &bytes);
	const int rc = newick_write(fp, root, t.length.data(), nodes, kid_off.data(), kid.data(), label, nullptr);
	fclose(fp);
	const std::string s(text, bytes);
	free(text);
	if (rc) return fail("newick refused", m);
	long open = 0, labels = 0;
	for (size_t i = 0; i < s.size(); i++) {
		if (s[i] == '(') open++;
		if (s[i] == ')' && --open < 0) return fail("newick parentheses", m);
		if (s[i] == 'n') labels++;
	}
	if (open != 0 || labels != (long) nodes || s.back() != ';') return fail("newick text", m);
	return 0;
}

static int refused(uint32_t m, const std::vector<uint32_t>& a, const std::vector<uint32_t>& b, uint32_t root, const char* what) {
	NjTree t;
	std::vector<int64_t> len(a.size() + 1, 65536);
	if (nj_orient(m, a.data(), b.data(), len.data(), root, t)) return fail(what, m);
	return 0;
}

int main() {
	std::mt19937 rng(2025);
	for (uint32_t m = 1; m <= 300; m += m < 12 ? 1 : 17)
		for (int round = 0; round < 8; round++)
			if (check_tree(m, rng)) return 1;
	// malformed edge lists (m = 4: 5 edges over 6 nodes)
	if (refused(4, {0, 1, 2, 3, 4}, {4, 4, 5, 5, 9}, 0, "an id out of range was accepted")) return 1;
	if (refused(4, {0, 1, 2, 3, 4}, {4, 4, 5, 5, 4}, 0, "a self loop was accepted")) return 1;
	if (refused(4, {0, 1, 2, 4, 4}, {4, 4, 5, 5, 5}, 0, "a doubled edge beside a loose leaf was accepted")) return 1;
	if (refused(4, {0, 1, 2, 3, 4}, {4, 4, 4, 4, 5}, 0, "a star was accepted")) return 1;
	if (refused(4, {0, 1, 2, 3, 4}, {4, 4, 5, 5, 5}, 4, "a root that is no leaf was accepted")) return 1;
	if (refused(4, {0, 1, 2, 3, 4}, {4, 4, 5, 5, 5}, 7, "a root out of range was accepted")) return 1;
	if (refused(0, {}, {}, 0, "m = 0 was accepted") || refused(NJ_MAX_M + 1, {}, {}, 0, "m past the limit was accepted")) return 1;
	if (refused(2, {0}, {0}, 0, "a loop on the one edge was accepted")) return 1;
	{                                                      // two components of the right degrees: 0-1 joined twice is impossible, so a 3-cycle of inner nodes
		if (refused(5, {0, 1, 5, 6, 7, 2, 3}, {5, 6, 6, 7, 5, 7, 4}, 0, "a cycle was accepted")) return 1;
	}
	// the node count
	uint64_t nodes = 0;
	const int32_t clone[9] = {3, -1, 3, 3, 0, 0, 3, 7, 3}, bad[2] = {0, -2};
	if (!nj_count_nodes(clone, 9, &nodes) || nodes != 9 + 3) return fail("node count", 9);
	if (!nj_count_nodes(clone, 0, &nodes) || nodes != 0) return fail("node count of nothing", 0);
	if (nj_count_nodes(bad, 2, &nodes)) return fail("a clone below -1 was accepted", 2);
	// the batches under every kind of knob
	const std::vector<uint32_t> size = {3, 5, 20, 2, 65, 4, 8};
	for (uint64_t knob : {1ull, 16ull, 2500ull, 1ull << 26}) {
		std::vector<uint32_t> end;
		link_batches(size, knob, end);
		if (end.empty() || end.back() != size.size()) return fail("batches cover", (size_t) knob);
	}
	// parents that are no forest, and a cycle the writer must not run around for ever
	const int32_t loop[3] = {1, 2, 0}, out_of_range[2] = {-1, 5}, self[2] = {-1, 1};
	size_t kid_off[4];
	uint32_t kid[3];
	if (!newick_children(out_of_range, 2, kid_off, kid) || !newick_children(self, 2, kid_off, kid)) return fail("bad parents were accepted", 2);
	if (newick_children(loop, 3, kid_off, kid)) return fail("a cycle's children", 3);
	const int64_t len3[3] = {0, 0, 0};
	char* text = nullptr;
	size_t bytes = 0;
	FILE* fp = open_memstream(&text, &bytes);
	const int rc = newick_write(fp, 0, len3, 3, kid_off, kid, label, nullptr);
	fclose(fp);
	free(text);
	if (!rc) return fail("a cycle was written", 3);
	puts("ok");
	return 0;
}
