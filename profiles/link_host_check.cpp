// link_host_check.cpp -- the host side of vdjx_lineage_link (vdjer_amd/csrc/vdjx_link.h: component order and batches) on the CPU, stand-alone,
// for a run under a sanitizer:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I vdjer_amd/csrc profiles/link_host_check.cpp -o link_host_check && ./link_host_check
// Random forests of roots (every root the smallest member of its component, items that take no part), the empty input, one component of
// everything, roots that are none; every knob from 1 up.  Each result is checked against a plain recount.  Prints "ok" and returns 0.
#include "vdjx_link.h"

#include <stdio.h>
#include <stdlib.h>

#include <map>
#include <random>

static int fail(const char* what, size_t n) {
	fprintf(stderr, "link_host_check: %s (n = %zu)\n", what, n);
	return 1;
}

static int check(const std::vector<uint32_t>& root) {
	const size_t n = root.size();
	LinkOrder o;
	if (!link_order(root.data(), n, o)) return fail("refused", n);
	std::map<uint32_t, std::vector<uint32_t>> want;          // root -> members, both ascending
	for (size_t i = 0; i < n; i++)
		if (root[i] != LINK_NO_ROOT) want[root[i]].push_back((uint32_t) i);
	if (o.clones_single != want.size()) return fail("clones_single", n);
	size_t k = 0, at = 0;
	uint32_t largest = 0;
	for (const auto& w : want) {
		if (w.second.size() < 2) continue;
		if (k >= o.size.size() || o.first[k] != at || o.size[k] != w.second.size()) return fail("component", n);
		for (size_t j = 0; j < w.second.size(); j++)
			if (o.member[at + j] != w.second[j]) return fail("member", n);
		largest = std::max(largest, (uint32_t) w.second.size());
		at += w.second.size();
		k++;
	}
	if (k != o.size.size() || at != o.member.size() || largest != o.largest) return fail("totals", n);
	for (uint64_t knob : {1ull, 2ull, 4ull, 5ull, 9ull, 64ull, 1000ull, 1ull << 26, 1ull << 28}) {
		std::vector<uint32_t> end;
		link_batches(o.size, knob, end);
		if (o.size.empty() != end.empty() || (!end.empty() && end.back() != o.size.size())) return fail("batches cover", n);
		size_t b0 = 0;
		for (size_t b = 0; b < end.size(); b++) {
			if (end[b] <= b0) return fail("empty batch", n);
			uint64_t cells = 0;
			for (size_t q = b0; q < end[b]; q++) cells += (uint64_t) o.size[q] * o.size[q];
			if (cells > knob && end[b] - b0 != 1) return fail("batch over the knob", n);
			if (end[b] < o.size.size() && cells + (uint64_t) o.size[end[b]] * o.size[end[b]] <= knob) return fail("batch closed early", n);
			b0 = end[b];
		}
	}
	return 0;
}

int main() {
	std::mt19937 rng(2024);
	if (check({})) return 1;
	if (check(std::vector<uint32_t>(100, LINK_NO_ROOT))) return 1;
	if (check(std::vector<uint32_t>(5000, 0u))) return 1;
	for (int round = 0; round < 300; round++) {
		const size_t n = 1 + rng() % 3000;
		const uint32_t spread = 1 + rng() % 40;
		std::vector<uint32_t> root(n);
		for (size_t i = 0; i < n; i++) {
			const uint32_t pick = rng() % spread;
			if (pick == 0 && rng() % 3 == 0) { root[i] = LINK_NO_ROOT; continue; }
			size_t r = i >= pick ? i - pick : i;                 // an earlier item's root, or its own
			while (r < i && root[r] == LINK_NO_ROOT) r++;
			root[i] = r == i ? (uint32_t) i : root[r];
		}
		if (check(root)) return 1;
	}
	LinkOrder o;
	const uint32_t bad1[3] = {0, 2, 2}, bad3[3] = {1, 1, 2};
	if (link_order(bad1, 3, o) || link_order(bad3, 3, o)) return fail("a root past its item was accepted", 3);
	puts("ok");
	return 0;
}
