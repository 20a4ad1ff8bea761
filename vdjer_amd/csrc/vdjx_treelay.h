// vdjx_treelay.h -- the host's layout of the clones' members as rows: what vdjx_tree.hip and vdjx_nj.hip share (gfx950 only).
//
// The host sorts the (clone, index) keys -- per item --, computes each clone's common window and lays the members out in clone order
// ("rows"); inside a clone the rows are in index order.  A row is `words` {bases, mask} pairs in vdjx_hamming.h's format.
//   tree_check_contigs   what every entry refuses about the contigs
//   tree_keys            clone << 20 | index of every member, sorted
//   tree_lay             the rows of the sorted keys: the windows, where each member's window starts, the packed layout, the roots
// Everything here has internal linkage.
#pragma once
#include "vdjx_common.h"

#include <string.h>

#include <algorithm>
#include <vector>

struct TreeRow { u64 at; u32 wbase, w; };                                      // where the window's characters start; the row's first word; bases
static_assert(sizeof(TreeRow) == 16, "uploaded as it is");

struct TreeClone { u32 first, m, words, wbase, root, w; };                    // rows [first, first + m), `words` pairs each from pair `wbase` on; the root's row; bases

// what both entries refuse about the contigs
static int tree_check_contigs(const char* who, const char* contigs, size_t n, int len) {
	if (n >= (1ull << 20)) { vdjx_set_error("%s: %zu items (at most 2^20 - 1 per call)", who, n); return VDJX_EINVAL; }
	if (len < 1 || len >= 4096) { vdjx_set_error("%s: contigs of %d characters (1 .. 4095)", who, len); return VDJX_EINVAL; }
	if (memchr(contigs, 0, n * (size_t) len)) { vdjx_set_error("%s: contigs of unequal length (a NUL inside the %zu x %d characters)", who, n, len); return VDJX_EINVAL; }
	return VDJX_OK;
}

// clone << 20 | index of every member, sorted: the clone order, the members of a clone in index order
static int tree_keys(const char* who, size_t n, int len, const int32_t* clone, const int32_t* anchor, std::vector<u64>& keys) {
	for (size_t i = 0; i < n; i++) {
		if (clone[i] < -1) { vdjx_set_error("%s: item %zu has clone %d (a key >= 0, or -1 for no part)", who, i, clone[i]); return VDJX_EINVAL; }
		if (clone[i] < 0) continue;
		if (anchor[i] < 0 || anchor[i] > len) { vdjx_set_error("%s: item %zu has its anchor at %d (0 .. %d)", who, i, anchor[i], len); return VDJX_EINVAL; }
		keys.push_back((u64) (u32) clone[i] << 20 | (u64) i);
	}
	std::sort(keys.begin(), keys.end());
	return VDJX_OK;
}

// the rows of the sorted keys: every clone's common window, where each member's window starts, the packed layout
struct TreeLay {
	std::vector<TreeClone> clones;
	std::vector<TreeRow> ri;                              // rows + 1: the last is k_tree_pack's sentinel
	std::vector<u32> row_item;
	u64 total = 0, cells = 0;                             // {bases, mask} pairs in all; the squared sizes of the clones of two and more
	u32 largest = 0;
};
static int tree_lay(const char* who, const std::vector<u64>& keys, int len, const int32_t* clone, const int32_t* anchor, const uint32_t* prio, TreeLay& L) {
	const u32 rows = (u32) keys.size();
	L.ri.resize(rows + 1);
	L.row_item.resize(rows);
	for (u32 r0 = 0; r0 < rows;) {
		u32 r1 = r0;
		int a = len, b = len;                               // the common window: a bases before the anchor, b from it on
		while (r1 < rows && (keys[r1] >> 20) == (keys[r0] >> 20)) {
			const u32 i = (u32) (keys[r1] & 0xFFFFFu);
			a = std::min(a, (int) anchor[i]);
			b = std::min(b, len - (int) anchor[i]);
			r1++;
		}
		const u32 w = (u32) (a + b), m = r1 - r0;
		if (w == 0) {
			vdjx_set_error("%s: clone %d has an empty window (a member's anchor at 0 and a member's at %d)", who, clone[keys[r0] & 0xFFFFFu], len);
			return VDJX_EINVAL;
		}
		const u32 words = (w + 31u) / 32u;
		if (L.total + (u64) m * words > 0xFFFFFFFFull) { vdjx_set_error("%s: more than 2^32 packed words", who); return VDJX_ELIMIT; }
		u32 root = r0;
		for (u32 r = r0; r < r1; r++) {
			const u32 i = (u32) (keys[r] & 0xFFFFFu);
			L.row_item[r] = i;
			L.ri[r] = {(u64) i * (u64) len + (u64) (anchor[i] - a), (u32) L.total + (r - r0) * words, w};
			if (prio && prio[i] < prio[L.row_item[root]]) root = r;      // (rows are in index order: a tie keeps the smaller index)
		}
		L.clones.push_back({r0, m, words, (u32) L.total, root, w});
		L.total += (u64) m * words;
		L.largest = std::max(L.largest, m);
		if (m > 1) L.cells += (u64) m * m;
		r0 = r1;
	}
	L.ri[rows] = {0, (u32) L.total, 0};
	return VDJX_OK;
}
