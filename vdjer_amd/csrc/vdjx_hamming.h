// vdjx_hamming.h -- packed rows, their Hamming distance and the work items of an all-pairs pass: what vdjx_lineage.hip and vdjx_tree.hip share (gfx950 only, wave64).
//
// The format: a row is a run of {bases, mask} pairs of 64-bit words, 32 bases per word, 2 bits each (A0 T1 C2 G3, base k of a word in
// bits 2k+1, 2k); the mask has bit 2k+1 set where base k is not ACGT.  Words past the row's end, and bits past it, are 0 in both.
//   ham_pack_word    the pair of word w from a callable pos -> char
//   ham_word         the distance of two pairs: popcount((((x ^ y) | ((x ^ y) << 1)) & 0xAAAA...) | mx | my).  The upper bit of a base's
//                    two collects the difference, so the shift never has to cross the halves of a 64-bit word and is one v_lshl_or_b32
//                    per half: ten integer instructions per word and lane
//   HamItem          one wave's work: a block of up to 64 rows (one per lane) against a column slice of the same group, three words
//                    of the user's.  ham_slice_width and ham_slice_items (host) cut a group into them
//   HAM_CASES_8/16   the switch over an item's uniform word count into the unrolled bodies of a kernel's register path: there the lane
//                    keeps its row's W words in registers, the columns go through LDS in tiles and are read back as one 16-byte
//                    {bases, mask} broadcast per word (lin_item in vdjx_lineage.hip, tree_item in vdjx_tree.hip: the two loops are kept
//                    apart, profiles/hamming_engine_refactor_check.md says why)
// Everything here has internal linkage.
#pragma once
#include "vdjx_common.h"

#include <algorithm>
#include <vector>

#define HAM_MA 0xAAAAAAAAu               // the upper bit of every base's two
#define HAM_ROWS 64u                     // rows per work item: one per lane
#define HAM_TARGET_ITEMS 4096u           // work items aimed at: 4 waves on each of the 1,024 SIMDs

struct HamItem { u32 row0, row_end, col0, col_end, words, u[3]; };      // rows [row0, row_end) (at most 64) against columns [col0, col_end)
struct HamGroup { u32 first, rows, words, u[3]; };                       // rows [first, first + rows) are compared all against all
static_assert(sizeof(HamItem) == 32, "uploaded as it is");

namespace {

// the work items: (group, row block, column slice).  The slice is a whole number of 64 columns, as wide as it takes for about
// HAM_TARGET_ITEMS items in all: 64 where the input is small (a group of 2,000 rows: 32 row blocks x 32 slices).  cells = the sum of rows^2.
inline u32 ham_slice_width(u64 cells) {
	const u64 per = (cells + (u64) HAM_ROWS * HAM_TARGET_ITEMS - 1) / ((u64) HAM_ROWS * HAM_TARGET_ITEMS);
	return (u32) std::max<u64>(HAM_ROWS, (per + HAM_ROWS - 1) / HAM_ROWS * HAM_ROWS);
}

// appends the items of one group, `slice` from ham_slice_width over all the groups of the launch
inline void ham_slice_items(const HamGroup& g, u32 slice, std::vector<HamItem>& items) {
	const u32 end = g.first + g.rows;
	for (u32 r0 = g.first; r0 < end; r0 += HAM_ROWS)
		for (u32 c0 = g.first; c0 < end; c0 += slice)
			items.push_back({r0, std::min(end, r0 + HAM_ROWS), c0, std::min(end, c0 + slice), g.words, {g.u[0], g.u[1], g.u[2]}});
}

template <typename F>
__device__ inline ulonglong2 ham_pack_word(F fetch, u32 w, u32 len) {
	u64 x = 0, m = 0;
	for (u32 k = 0; k < 32u; k++) {
		const u32 pos = w * 32u + k;
		if (pos >= len) break;
		const char ch = fetch(pos);
		const u32 code = ch == 'A' ? 0u : ch == 'T' ? 1u : ch == 'C' ? 2u : ch == 'G' ? 3u : 4u;
		if (code < 4u) x |= (u64) code << (2u * k);
		else m |= 2ull << (2u * k);
	}
	return make_ulonglong2(x, m);
}

__device__ inline u32 ham_word(const u64 x, const u64 m, const ulonglong2 q) {
	const u64 t = x ^ q.x, mm = m | q.y;
	const u32 lo = (u32) t, hi = (u32) (t >> 32);
	return (u32) __popc(((lo | (lo << 1)) & HAM_MA) | (u32) mm) + (u32) __popc(((hi | (hi << 1)) & HAM_MA) | (u32) (mm >> 32));
}

}  // namespace

// `case 1 ... 8 (16)` of a switch over a wave-uniform word count.  The macro declares the constant W inside each case, for the body
// to use as a template argument: a body must not rely on a W of its own
#define HAM_CASE(n, ...) case n: { constexpr int W = n; __VA_ARGS__; } break;
#define HAM_CASES_8(...) HAM_CASE(1, __VA_ARGS__) HAM_CASE(2, __VA_ARGS__) HAM_CASE(3, __VA_ARGS__) HAM_CASE(4, __VA_ARGS__) \
	HAM_CASE(5, __VA_ARGS__) HAM_CASE(6, __VA_ARGS__) HAM_CASE(7, __VA_ARGS__) HAM_CASE(8, __VA_ARGS__)
#define HAM_CASES_16(...) HAM_CASES_8(__VA_ARGS__) HAM_CASE(9, __VA_ARGS__) HAM_CASE(10, __VA_ARGS__) HAM_CASE(11, __VA_ARGS__) HAM_CASE(12, __VA_ARGS__) \
	HAM_CASE(13, __VA_ARGS__) HAM_CASE(14, __VA_ARGS__) HAM_CASE(15, __VA_ARGS__) HAM_CASE(16, __VA_ARGS__)
