// split_host_check.cpp -- the host side of vdjx_tree_split_support / vdjx_tree_split_compare (vdjer_amd/csrc/vdjx_split_host.h: a rooted
// tree's clades as bitsets, the canonical side, the signatures, the scored nodes) on the CPU, stand-alone, for a run under a sanitizer:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I vdjer_amd/csrc profiles/split_host_check.cpp -o split_host_check && ./split_host_check
// Random binary trees of 3 .. 300 leaves (and sizes around every multiple of 64 up to 4,096 once) rooted at a random leaf: every clade is
// recounted by walking each leaf to the root; a clade made canonical against any leaf never holds that leaf and is the clade or its
// complement within m bits (no bit past m); the scored nodes are the m - 3 inferred nodes other than the root's child, sorted by signature,
// their clades distinct; the same tree rooted at another leaf has the same scored clades against the first root.  Prints "ok", returns 0.
#include "vdjx_split_host.h"

#include <stdio.h>

#include <random>
#include <set>

static int fail(const char* what, size_t m) {
	fprintf(stderr, "split_host_check: %s (m = %zu)\n", what, m);
	return 1;
}

// leaves 0 .. m - 1, inner nodes m .. 2m - 3: every new leaf into a random edge
static void random_edges(uint32_t m, std::mt19937& rng, std::vector<uint32_t>& a, std::vector<uint32_t>& b) {
	a.clear(); b.clear();
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
}

static bool bit(const uint64_t* c, uint32_t v) { return c[v >> 6] >> (v & 63u) & 1u; }

static int check(uint32_t m, std::mt19937& rng) {
	std::vector<uint32_t> a, b;
	random_edges(m, rng, a, b);
	const std::vector<int64_t> len(a.size(), 0);
	const uint32_t root = rng() % m, other = (root + 1 + rng() % (m - 1)) % m, words = split_words(m);
	NjTree t, t2;
	if (!nj_orient(m, a.data(), b.data(), len.data(), root, t) || !nj_orient(m, a.data(), b.data(), len.data(), other, t2)) return fail("edges refused", m);
	std::vector<uint64_t> cl, cl2, want((size_t) (m - 2) * words, 0);
	split_clades(m, t, cl);
	if (cl.size() != want.size()) return fail("size", m);
	for (uint32_t leaf = 0; leaf < m; leaf++)
		for (int32_t v = t.parent[leaf]; v >= 0; v = t.parent[v])
			if ((uint32_t) v >= m) want[(size_t) ((uint32_t) v - m) * words + (leaf >> 6)] |= 1ull << (leaf & 63u);
	if (cl != want) return fail("clades", m);
	for (uint32_t v = m; v < 2 * m - 2; v++) {                  // canonical against a random leaf
		const uint32_t against = rng() % m;
		std::vector<uint64_t> c(cl.begin() + (size_t) (v - m) * words, cl.begin() + (size_t) (v - m + 1) * words);
		const bool held = bit(c.data(), against);
		split_canonical(m, against, c.data());
		for (uint32_t x = 0; x < 64 * words; x++)
			if (bit(c.data(), x) != (x < m && (bit(want.data() + (size_t) (v - m) * words, x) != held))) return fail("canonical", m);
	}
	if (m < 4) return 0;
	std::vector<SplitScored> sc, sc2;
	split_scored(m, root, t.root_kid, cl, sc);
	split_clades(m, t2, cl2);
	split_scored(m, root, t2.root_kid, cl2, sc2);             // the tree rooted elsewhere, against the first root
	if (sc.size() != m - 3 || sc2.size() != m - 3) return fail("scored count", m);
	std::set<std::vector<uint64_t>> mine, theirs;
	for (size_t i = 0; i < sc.size(); i++) {
		if (i && sc[i - 1].sig > sc[i].sig) return fail("order", m);
		if (sc[i].node == t.root_kid || sc[i].node < m || sc[i].node >= 2 * m - 2) return fail("scored node", m);
		const uint64_t* c = cl.data() + (size_t) (sc[i].node - m) * words;
		if (sc[i].sig != split_sig(m, c) || bit(c, root)) return fail("signature", m);
		mine.insert(std::vector<uint64_t>(c, c + words));
		const uint64_t* c2 = cl2.data() + (size_t) (sc2[i].node - m) * words;
		theirs.insert(std::vector<uint64_t>(c2, c2 + words));
	}
	if (mine.size() != m - 3) return fail("clades not distinct", m);
	if (mine != theirs) return fail("another root, other splits", m);
	return 0;
}

int main() {
	std::mt19937 rng(27);
	for (int round = 0; round < 400; round++)
		if (check(3 + rng() % 298, rng)) return 1;
	for (uint32_t m = 64; m <= 4096; m += 64)
		for (uint32_t d = 0; d < 3; d++)
			if (m - 1 + d <= NJ_MAX_M && check(m - 1 + d, rng)) return 1;
	puts("ok");
	return 0;
}
