// vdjx_link.h -- the host side of complete and average linkage (vdjx_lineage_link, vdjx_lineage.hip): the single-linkage components in the
// order the device agglomerates them, and their batches.  Plain C++, no GPU: profiles/link_host_check.cpp runs both under a sanitizer.
//
//   link_order     from every item's root (the flattened union-find of the pair pass: the smallest member of its component, LINK_NO_ROOT for
//                  an item that takes no part): the components of two and more members in the order of their smallest member, the members
//                  of each by index.  Per item, three passes
//   link_batches   whole components, in that order, in batches of at most `knob` matrix cells (a component of m members has m * m); a
//                  component of more cells than the knob goes alone
// Everything here has internal linkage.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#define LINK_NO_ROOT 0xFFFFFFFFu
#define LINK_MAX_M 4096u                 // members of a component under complete or average linkage

struct LinkOrder {
	std::vector<uint32_t> first, size;   // per component: where its members start in member[], how many they are
	std::vector<uint32_t> member;        // item indices, component after component
	uint32_t clones_single = 0, largest = 0;
};

namespace {

// false: a root that is not an item, or not its own root (never from the device; the stand-alone check feeds such input)
inline bool link_order(const uint32_t* root, size_t n, LinkOrder& o) {
	o = LinkOrder();
	std::vector<uint32_t> cnt(n, 0u), at(n, LINK_NO_ROOT);
	for (size_t i = 0; i < n; i++) {
		const uint32_t r = root[i];
		if (r == LINK_NO_ROOT) continue;
		if (r > i || root[r] != r) return false;
		cnt[r]++;
	}
	uint32_t total = 0;
	for (size_t i = 0; i < n; i++) {
		if (root[i] != (uint32_t) i) continue;
		o.clones_single++;
		if (cnt[i] < 2u) continue;
		at[i] = total;
		o.first.push_back(total);
		o.size.push_back(cnt[i]);
		o.largest = std::max(o.largest, cnt[i]);
		total += cnt[i];
	}
	o.member.resize(total);
	for (size_t i = 0; i < n; i++) {
		const uint32_t r = root[i];
		if (r != LINK_NO_ROOT && at[r] != LINK_NO_ROOT) o.member[at[r]++] = (uint32_t) i;
	}
	return true;
}

// end[b]: one past the last component of batch b
inline void link_batches(const std::vector<uint32_t>& size, uint64_t knob, std::vector<uint32_t>& end) {
	end.clear();
	uint64_t cur = 0;
	for (size_t k = 0; k < size.size(); k++) {
		const uint64_t cells = (uint64_t) size[k] * size[k];
		if (cur && cur + cells > knob) {
			end.push_back((uint32_t) k);
			cur = 0;
		}
		cur += cells;
	}
	if (!size.empty()) end.push_back((uint32_t) size.size());
}

}  // namespace
