// sankoff_host_check.cpp -- the host side of vdjx_tree_sankoff and vdjx_sankoff_costs (vdjer_amd/csrc/vdjx_sankoff_host.h: the check of a
// cost matrix and the collapse of a targeting model's 5-mer weights to a 4 x 4 matrix) on the CPU, stand-alone, for a run under a sanitizer:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I vdjer_amd/csrc profiles/sankoff_host_check.cpp -o sankoff_host_check && ./sankoff_host_check
// Matrix validation: the unit matrix, every cell moved out of its range in turn, the edges of the range.  The collapse: on random weights
// every matrix passes the check, the smallest and largest cell are the reported ones and a heavier substitution is never dearer than a
// lighter one; zero rows and an all-zero model (w' = 1: the uniform matrix of 1000); saturated weights whose 64-bit sums exceed 2^32 (the
// uniform matrix again, and with one centre base saturated a cheaper row); one substitution with all the weight (the clamp at 65535 is
// not reached: the ratio's logarithm is bounded).  Every buffer is heap-allocated at its exact size.  Prints "ok" and returns 0.
#include "vdjx_sankoff_host.h"

#include <stdio.h>

#include <random>
#include <vector>

static int fail(const char* what, int i) {
	fprintf(stderr, "sankoff_host_check: %s (%d)\n", what, i);
	return 1;
}

struct Collapsed { std::vector<uint32_t> cost; double mean; uint32_t lo, hi; };

static Collapsed collapse(const std::vector<uint32_t>& weight) {
	Collapsed r;
	r.cost.assign(16, 0xDEADBEEFu);
	sk_collapse(weight.data(), r.cost.data(), &r.mean, &r.lo, &r.hi);
	return r;
}

static bool uniform(const Collapsed& r) {
	for (int i = 0; i < 16; i++)
		if (r.cost[i] != ((i >> 2) == (i & 3) ? 0u : 1000u)) return false;
	return r.lo == 1000 && r.hi == 1000;
}

int main() {
	std::vector<uint32_t> c(16);
	sk_unit_costs(c.data());
	if (sk_check_costs(c.data()) != -1) return fail("the unit matrix", 0);
	for (int i = 0; i < 16; i++) {
		const bool diag = (i >> 2) == (i & 3);
		std::vector<uint32_t> bad = c;
		bad[i] = diag ? 1u : 0u;
		if (sk_check_costs(bad.data()) != i) return fail("a cell below its range", i);
		bad[i] = diag ? 0xFFFFFFFFu : 65536u;
		if (sk_check_costs(bad.data()) != i) return fail("a cell above its range", i);
		bad[i] = diag ? 0u : 65535u;
		if (sk_check_costs(bad.data()) != -1) return fail("the largest cost", i);
	}
	std::vector<uint32_t> two = c;
	two[7] = 0; two[2] = 70000;
	if (sk_check_costs(two.data()) != 2) return fail("the first of two bad cells", 2);

	std::mt19937 rng(2029);
	for (int round = 0; round < 200; round++) {
		std::vector<uint32_t> w(1024 * 4);
		const uint32_t span = round % 3 == 0 ? 0xFFFFFFFFu : round % 3 == 1 ? 5000u : 3u;
		for (uint32_t& x : w) x = (uint32_t) (rng() % ((uint64_t) span + 1));
		if (round % 5 == 0)
			for (uint32_t row = 0; row < 1024; row += 1 + rng() % 3)
				for (int e = 0; e < 4; e++) w[row * 4 + e] = 0;      // zero rows
		const Collapsed r = collapse(w);
		if (sk_check_costs(r.cost.data()) != -1) return fail("a collapsed matrix is no cost matrix", round);
		uint64_t sum[16] = {0};
		for (uint32_t row = 0; row < 1024; row++)
			for (uint32_t e = 0; e < 4; e++) sum[((row >> 4) & 3u) * 4u + e] += w[row * 4 + e];
		uint32_t lo = 65535, hi = 1;
		for (int i = 0; i < 16; i++) {
			if ((i >> 2) == (i & 3)) continue;
			lo = r.cost[i] < lo ? r.cost[i] : lo;
			hi = r.cost[i] > hi ? r.cost[i] : hi;
			for (int j = 0; j < 16; j++)
				if ((j >> 2) != (j & 3) && sum[i] > sum[j] && r.cost[i] > r.cost[j]) return fail("a heavier substitution is dearer", round);
		}
		if (lo != r.lo || hi != r.hi || !(r.mean > 0.0)) return fail("the reported mean, smallest and largest cell", round);
	}
	if (!uniform(collapse(std::vector<uint32_t>(1024 * 4, 0u)))) return fail("the all-zero model", 0);
	if (!uniform(collapse(std::vector<uint32_t>(1024 * 4, 0xFFFFFFFFu)))) return fail("the saturated model (sums of 256 x (2^32 - 1))", 0);
	{
		std::vector<uint32_t> w(1024 * 4, 1u);                  // centre G saturated: its row is cheaper than every other cell
		for (uint32_t row = 0; row < 1024; row++)
			if (((row >> 4) & 3u) == 2u)
				for (int e = 0; e < 4; e++) w[row * 4 + e] = 0xFFFFFFFFu;
		const Collapsed r = collapse(w);
		if (sk_check_costs(r.cost.data()) != -1) return fail("one saturated centre", 0);
		for (int i = 0; i < 16; i++)
			if ((i >> 2) != (i & 3) && (i >> 2) != 2 && r.cost[i] <= r.cost[8]) return fail("one saturated centre: the other rows are dearer", i);
		if (r.cost[8] != r.cost[9] || r.cost[9] != r.cost[11] || r.cost[10] != 0) return fail("one saturated centre: its row", 0);
	}
	{
		std::vector<uint32_t> w(1024 * 4, 0u);                  // one substitution has all the weight: the eleven others are w' = 1
		w[((1u << 4) | 5u) * 4 + 3] = 0xFFFFFFFFu;
		const Collapsed r = collapse(w);
		if (sk_check_costs(r.cost.data()) != -1 || r.cost[7] != 1u || r.lo != 1u) return fail("one substitution with all the weight", (int) r.cost[7]);
		for (int i = 0; i < 16; i++)
			if ((i >> 2) != (i & 3) && i != 7 && r.cost[i] != r.hi) return fail("the eleven others are equal", i);
	}
	puts("ok");
	return 0;
}
