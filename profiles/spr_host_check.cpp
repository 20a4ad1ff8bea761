// spr_host_check.cpp -- the host side of vdjx_tree_spr (vdjer_amd/csrc/vdjx_spr_host.h: the candidates of a tree, the legality of a move and
// the move on a lineage's parents) on the CPU, stand-alone, for a run under a sanitizer:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I vdjer_amd/csrc profiles/spr_host_check.cpp -o spr_host_check && ./spr_host_check
// Random binary trees of 4 .. 300 leaves rooted at a random leaf.  On each: spr_candidates against the moves spr_legal admits, counted one by
// one (small trees) and against the sum over c of 2 (m - leaves(c)) - 4 with the leaves counted by a walk of its own (every tree); then
// random legal (c, y): mp_orient accepts every result, its children ascend, the inverse regraft (c, s) is legal and restores the parents.
// Moves no search proposes are refused by spr_legal.  Prints "ok" and returns 0.
#include "vdjx_spr_host.h"

#include <stdio.h>

#include <random>

static int fail(const char* what, size_t m) {
	fprintf(stderr, "spr_host_check: %s (m = %zu)\n", what, m);
	return 1;
}

// leaves 0 .. m - 1, inner nodes m .. 2m - 3: every new leaf into a random edge, then rooted at `root` through nj_orient
static bool random_parents(uint32_t m, uint32_t root, std::mt19937& rng, std::vector<int32_t>& parent) {
	std::vector<uint32_t> a, b;
	auto add = [&](uint32_t x, uint32_t y) { a.push_back(x); b.push_back(y); };
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
	std::vector<int64_t> len(a.size() + 1, 0);
	NjTree t;
	if (!nj_orient(m, a.data(), b.data(), len.data(), root, t)) return false;
	parent = t.parent;
	return true;
}

// the leaves below v, by walking every leaf up to the root
static std::vector<uint32_t> leaves_below(uint32_t m, uint32_t root, const std::vector<int32_t>& parent) {
	std::vector<uint32_t> out(2 * (size_t) m - 2, 0);
	for (uint32_t l = 0; l < m; l++) {
		if (l == root) continue;
		for (uint32_t v = l; v != root; v = (uint32_t) parent[v]) out[v]++;
	}
	return out;
}

int main() {
	std::mt19937 rng(2028);
	for (uint32_t m = 4; m <= 300; m += m < 12 ? 1 : 17)
		for (int round = 0; round < 6; round++) {
			const uint32_t root = rng() % m, nodes = 2 * m - 2;
			std::vector<int32_t> parent;
			if (!random_parents(m, root, rng, parent)) return fail("the generator", m);
			for (int move = 0; move < 25; move++) {
				NjTree t;
				if (mp_orient(m, root, parent.data(), t) != MP_OK) return fail("a tree was refused", m);
				const std::vector<uint32_t> below = leaves_below(m, root, parent);
				uint64_t want = 0;
				for (uint32_t c = 0; c < nodes; c++)
					if (c != root && c != t.root_kid) want += 2ull * (m - below[c]) - 4;
				if (spr_candidates(m, root, t) != want) return fail("the candidates of a tree", m);
				if (m <= 40 && move < 3) {
					uint64_t legal = 0;
					for (uint32_t c = 0; c < nodes; c++)
						for (uint32_t y = 0; y < nodes; y++) legal += spr_legal(m, root, parent.data(), c, y);
					if (legal != want) return fail("the legal moves, one by one", m);
				}
				uint32_t c, y;
				do { c = rng() % nodes; y = rng() % nodes; } while (!spr_legal(m, root, parent.data(), c, y));
				const std::vector<int32_t> before = parent;
				const uint32_t s = spr_apply(m, root, parent.data(), c, y);
				if (mp_orient(m, root, parent.data(), t) != MP_OK) return fail("a move's result is no tree", m);
				for (uint32_t v = m; v < nodes; v++)
					if (t.kid[2 * (size_t) (v - m)] >= t.kid[2 * (size_t) (v - m) + 1]) return fail("children ascend", m);
				if ((uint32_t) parent[c] != (uint32_t) before[c] || (uint32_t) parent[y] != (uint32_t) before[c]) return fail("c and y under p", m);
				if (!spr_legal(m, root, parent.data(), c, s)) return fail("the inverse is no candidate", m);
				std::vector<int32_t> back = parent;
				if (spr_apply(m, root, back.data(), c, s) != y) return fail("the inverse's sibling", m);
				back[root] = before[root];
				if (back != before) return fail("the inverse regraft does not restore the parents", m);
			}
		}
	// m = 5, root 0: the caterpillar 0 <- 5 <- {1, 6}, 6 <- {2, 7}, 7 <- {3, 4}
	const std::vector<int32_t> cat = {-1, 5, 6, 7, 7, 0, 5, 6};
	const struct { uint32_t c, y; bool ok; } moves[] = {{0, 1, false}, {5, 1, false}, {1, 0, false}, {1, 6, false}, {1, 5, false}, {6, 7, false}, {6, 3, false},
	                                                    {6, 6, false}, {3, 4, false}, {3, 7, false}, {8, 1, false}, {1, 8, false}, {1, 2, true}, {1, 7, true},
	                                                    {3, 5, true}, {3, 1, true}, {7, 1, true}, {7, 5, true}, {6, 1, false}};
	for (const auto& q : moves)
		if (spr_legal(5, 0, cat.data(), q.c, q.y) != q.ok) return fail("a move by hand", q.c * 10 + q.y);
	NjTree t;
	if (mp_orient(5, 0, cat.data(), t) != MP_OK || spr_candidates(5, 0, t) != 4 + 4 + 4 + 4 + 0 + 2) return fail("the caterpillar's candidates", 5);
	if (spr_candidates(3, 0, t) != 0) return fail("a lineage of three", 3);
	puts("ok");
	return 0;
}
