// vdjx_sankoff_host.h -- the host side of vdjx_tree_sankoff and vdjx_sankoff_costs (vdjx_sankoff.hip): the cost matrix.  Plain C++, no GPU:
// profiles/sankoff_host_check.cpp runs it under a sanitizer.  The start trees are vdjx_tree_mp's (vdjx_mp_host.h, unchanged).
//
//   sk_check_costs   the first cell of cost[16] (row-major, c[s][t]: a parent in state s over a child in state t) that is no cost: a diagonal
//                    cell other than 0 or an off-diagonal cell outside 1 .. SK_MAX_COST; -1 if there is none
//   sk_unit_costs    every off-diagonal cell 1: what a NULL matrix means (Fitch's count)
//   sk_collapse      vdjx_sankoff_costs' arithmetic: the 5-mer targeting weights collapsed to centre base -> new base, -log10 of the share,
//                    normalised to a mean of 1, in thousandths.  One float64 operation per statement and the sum in index order, as
//                    vdjx_lineage_distance_table does it: the Python restatement (tests/test_tree_sankoff_cpu.py) gives the same integers
// Everything here has internal linkage.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#define SK_MAX_COST 65535u

namespace {

inline int sk_check_costs(const uint32_t* cost) {
	for (int i = 0; i < 16; i++) {
		const bool diag = (i >> 2) == (i & 3);
		if (diag ? cost[i] != 0 : (cost[i] < 1 || cost[i] > SK_MAX_COST)) return i;
	}
	return -1;
}

inline void sk_unit_costs(uint32_t* cost) {
	for (int i = 0; i < 16; i++) cost[i] = (i >> 2) == (i & 3) ? 0u : 1u;
}

// weight[1024][4]: row = the 5-mer in base 4 (its centre base is (row >> 4) & 3), column = the new base
inline void sk_collapse(const uint32_t* weight, uint32_t* cost, double* mean_out, uint32_t* lo_out, uint32_t* hi_out) {
	uint64_t Wc[16];
	for (int i = 0; i < 16; i++) Wc[i] = 0;
	for (uint32_t row = 0; row < 1024; row++)
		for (uint32_t e = 0; e < 4; e++) Wc[((row >> 4) & 3u) * 4u + e] += weight[row * 4u + e];
	uint64_t S = 0;
	for (int i = 0; i < 16; i++) {
		if ((i >> 2) == (i & 3)) continue;
		if (Wc[i] < 1) Wc[i] = 1;
		S += Wc[i];
	}
	double d[16], sum = 0.0;
	for (int i = 0; i < 16; i++) {
		d[i] = 0.0;
		if ((i >> 2) == (i & 3)) continue;
		const double ratio = (double) Wc[i] / (double) S;
		d[i] = -log10(ratio);
		sum += d[i];
	}
	const double mean = sum / 12.0;
	uint32_t lo = SK_MAX_COST, hi = 1u;
	for (int i = 0; i < 16; i++) {
		if ((i >> 2) == (i & 3)) { cost[i] = 0; continue; }
		const double scaled = 1000.0 * d[i];
		const double unit = scaled / mean;
		const double t = floor(unit + 0.5);
		const uint32_t cell = t < 1.0 ? 1u : t > 65535.0 ? SK_MAX_COST : (uint32_t) t;      // (mean > 0: one of twelve shares is at most 1/12)
		cost[i] = cell;
		if (cell < lo) lo = cell;
		if (cell > hi) hi = cell;
	}
	*mean_out = mean;
	*lo_out = lo;
	*hi_out = hi;
}

}  // namespace
