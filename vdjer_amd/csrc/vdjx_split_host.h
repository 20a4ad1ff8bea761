// vdjx_split_host.h -- the host side of vdjx_tree_split_support and vdjx_tree_split_compare (vdjx_nj.hip): a rooted lineage tree's clades
// as bitsets, their signatures and the exact match of two trees' clades.  Plain C++, no GPU: profiles/split_host_check.cpp runs it under
// a sanitizer.
//
//   split_words      ceil(m / 64): the 64-bit words of a clade over the local leaf ids 0 .. m - 1
//   split_clades     the clade (the leaves below) of every inferred node of an NjTree, by one pass over its post-order
//   split_canonical  a clade that holds the bit of leaf `root` is complemented within m bits: the side of the edge without that leaf
//   split_sig        what the device's look-up sorts and searches by: up to 64 members the one word itself, beyond that the wrap-around
//                    sum of mix64(leaf + 1) over the clade's leaves.  Never the answer: a hit counts after all words compare equal
//   split_scored     the scored nodes of a lineage of four and more: every inferred node but the root's child, sorted by (signature, node)
//   split_lineage    one lineage's nodes of a caller's parent[] as local parents (mp_local), checked and rooted (mp_orient)
// Everything here has internal linkage.
#pragma once
#include "vdjx_mp_host.h"

namespace {

inline uint64_t split_mix64(uint64_t x) {                 // splitmix64's output step: vdjx_tree_support's mix64
	uint64_t z = x + 0x9E3779B97F4A7C15ull;
	z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
	z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
	return z ^ (z >> 31);
}

inline uint32_t split_words(uint32_t m) { return (m + 63u) / 64u; }

// out[(v - m) * words + l]: word l of inferred node v's clade (m >= 3; t from mp_orient or nj_orient)
inline void split_clades(uint32_t m, const NjTree& t, std::vector<uint64_t>& out) {
	const uint32_t words = split_words(m);
	out.assign((size_t) (m - 2) * words, 0);
	for (const uint32_t v : t.order) {                     // children before parents
		uint64_t* mine = out.data() + (size_t) (v - m) * words;
		for (int k = 0; k < 2; k++) {
			const uint32_t c = t.kid[2 * (size_t) (v - m) + k];
			if (c < m) mine[c >> 6] |= 1ull << (c & 63u);
			else
				for (uint32_t l = 0; l < words; l++) mine[l] |= out[(size_t) (c - m) * words + l];
		}
	}
}

inline void split_canonical(uint32_t m, uint32_t root, uint64_t* clade) {
	if (!(clade[root >> 6] >> (root & 63u) & 1u)) return;
	const uint32_t words = split_words(m);
	for (uint32_t l = 0; l < words; l++) clade[l] = ~clade[l];
	if (m & 63u) clade[words - 1] &= (1ull << (m & 63u)) - 1;
}

inline uint64_t split_sig(uint32_t m, const uint64_t* clade) {
	if (m <= 64u) return clade[0];
	uint64_t s = 0;
	for (uint32_t v = 0; v < m; v++)
		if (clade[v >> 6] >> (v & 63u) & 1u) s += split_mix64((uint64_t) v + 1);
	return s;
}

struct SplitScored { uint64_t sig; uint32_t node; };      // node: the local id of an inferred node

// the scored nodes of a rooted lineage (m >= 4), their clades canonical against leaf `root` in clades[]; sorted by (sig, node)
inline void split_scored(uint32_t m, uint32_t root, uint32_t root_kid, std::vector<uint64_t>& clades, std::vector<SplitScored>& out) {
	const uint32_t words = split_words(m);
	out.clear();
	for (uint32_t v = m; v < 2 * m - 2; v++) {
		if (v == root_kid) continue;
		uint64_t* mine = clades.data() + (size_t) (v - m) * words;
		split_canonical(m, root, mine);
		out.push_back({split_sig(m, mine), v});
	}
	std::sort(out.begin(), out.end(), [](const SplitScored& a, const SplitScored& b) { return a.sig < b.sig || (a.sig == b.sig && a.node < b.node); });
}

// the lineage of rows [first, first + m) with the inferred slots n + a0 ..: its nodes' entries of parent[] as local ids, rooted at `root`
inline int split_lineage(const int32_t* parent, size_t n, const int32_t* item_row, const uint32_t* row_item, uint32_t first, uint32_t m, uint64_t a0,
                         uint32_t root, std::vector<int32_t>& lp, NjTree& t) {
	const uint32_t nl = m < 3 ? m : 2 * m - 2;
	lp.resize(nl);
	for (uint32_t v = 0; v < nl; v++) {
		const uint64_t s = v < m ? (uint64_t) row_item[first + v] : (uint64_t) n + a0 + (v - m);
		lp[v] = v == root ? -1 : mp_local(parent[s], n, item_row, first, m, a0);
	}
	return mp_orient(m, root, lp.data(), t);
}

}  // namespace
