// vdjx_sankoff_spr.hip -- subtree pruning and regrafting under a 4 x 4 cost matrix for the lineage trees (gfx950 only, wave64).
//
//   vdjx_tree_sankoff_spr  per lineage: from vdjx_tree_nj's tree or the caller's, vdjx_tree_spr's rounds -- score every candidate (c, y),
//                          apply the one of smallest key (W, c, y) while it lowers W -- under vdjx_tree_sankoff's weighted cost W(T), then
//                          that call's down pass on the final topology (the model: include/vdjx.h; in Python:
//                          tests/tree_sankoff_spr_model.py)
//
// Everything around the search is vdjx_tree_spr's (vdjx_spr.hip): the layout, the start's check, the batches, kid[2] and par of every
// inferred node, the parent of every leaf, the root's child.  What is stored per (inferred node, column) is vdjx_tree_sankoff's: the node's
// message H to its parent, one 16-byte vector (vdjx_sankoff_dev.h).  Fitch's root-independence does not hold for an asymmetric matrix, so
// a candidate is scored from the rooted identity
//     W(T after (c, y)) = sum over the columns of min_u (E'_y(u) + H_c(u) + H'_y(u))
// with H' the messages of T' (the tree without c's subtree, p dissolved: the stored H but on the path from g to the root) and E'_y(u) the
// cheapest cost of everything in T' outside y's subtree plus the edge into a node in state u placed directly above y:
//     E'_top(u) = c[b_root][u] (0 where the root's character is a wildcard),  E'_y(u) = min_v (E'_x(v) + H'_z(v) + c[v][u])
// for the children y, z of x.  A round of a batch:
//   k_sksp_score   the hot kernel, k_spr_score's shape.  One wave per (lineage, pruned node c), a lane per column, the lineage's column tiles
//                  in turn.  Per tile every node's message is copied into the slab (a 16-byte vector per (node, lane)), the walk from g to
//                  the root writes H' over the path, then a stackless pre-order walk of T' over kid / par (wave-uniform addresses, p
//                  transparent, c's subtree never entered) stores every node's E' OVER its H': a node's H' is last read when its parent is
//                  expanded, where its E' is made and its score formed, both vectors in hand.  The lanes' scores are summed over the wave
//                  (a 64-bit butterfly: 64 columns of a large lineage under large costs pass 2^32) and added into the node's 64-bit
//                  sum in LDS.  The slab is in LDS up to VDJX_SKSP_LDS_MEMBERS members (two geometries, below), in the
//                  workspace beyond (a slab per launched workgroup, the grid capped, a workgroup strides over the prunes).  After the
//                  last tile the wave reduces (sum - W's share, y) to c's key: a 64-bit delta beside a 32-bit c << 16 | y
//   k_sksp_pick    one workgroup per lineage still searching: the smallest key (delta, c, y); if the delta is negative all threads
//                  rewrite the stored messages on the path above the pruned place on the old links, one thread rewires kid, par, the
//                  leaves' parents and the root's child between two barriers, all threads rewrite the messages from the regrafted place
//                  up on the new links (a walk ends where a message comes out as stored); W, the moves and the still-searching counter
//                  follow
// The host reads one counter per round (page-locked) and stops at 0 or at max_rounds; it reads kid and par back, roots them (O(nodes)) and
// runs k_sk_down (vdjx_sankoff_dev.h) on them.  Integer only; no spin-wait; nothing waits for another workgroup.  Integer atomics are sums
// only.  Scratch comes from the context's workspace.
#include "vdjx_common.h"
#include "vdjx_fitch.h"
#include "vdjx_link.h"
#include "vdjx_mp_host.h"
#include "vdjx_sankoff_dev.h"
#include "vdjx_sankoff_host.h"
#include "vdjx_spr_host.h"
#include "vdjx_treelay.h"

#include <string.h>

static_assert(VDJX_SPR_MAX_MEMBERS <= NJ_MAX_M, "a searched lineage is one vdjx_tree_nj takes");
static_assert(2u * VDJX_SPR_MAX_MEMBERS - 2u < 65536u, "c and y share a 32-bit word, 16 bits each");
// a column's quantities -- a message, an E', a candidate's cost, and the sums inside a min-plus step before the minimum is taken -- are
// costs of at most all 2m - 2 edges: 32 bits hold them
static_assert((unsigned long long) (2u * VDJX_SPR_MAX_MEMBERS - 2u) * SK_MAX_COST < (1ull << 31), "per-column quantities fit 31 bits");
#define SKSP_LDS_MEMBERS_8 10u           // up to it: a slab of at most 18 KiB, 8 waves per CU
#define VDJX_SKSP_LDS_MEMBERS 32u        // the largest lineage whose slab k_sksp_score keeps in LDS (below 64 KiB, 2 waves per CU)
#define SKSP_SLAB_WGS 256u               // beyond it: the workgroups launched, each with a slab in the workspace (one per CU)
#define SKSP_PICK_T 256
#define SKSP_SUM_NONE 0xFFFFFFFFFFFFFFFFull   // a sum no tile has added to: the node is no y of this prune
#define SKSP_KEY_NONE 0x7FFFFFFFFFFFFFFFll
// per node of a lineage: 1 KiB of slab (16 bytes per lane) and a 64-bit sum
#define SKSP_NODE_LDS_BYTES 1032u
static_assert((2u * SKSP_LDS_MEMBERS_8 - 2u) * SKSP_NODE_LDS_BYTES <= 20480u, "8 waves per CU keep their slabs in 160 KiB of LDS");
static_assert((2u * VDJX_SKSP_LDS_MEMBERS - 2u) * SKSP_NODE_LDS_BYTES <= 65536u, "a workgroup's slab stays below 64 KiB: 2 waves per CU");
static_assert(2u * VDJX_SPR_MAX_MEMBERS * (SKSP_NODE_LDS_BYTES - 1024u) <= 65536u, "the sums of the largest lineage fit a workgroup's LDS");

// min_v (T[v] + c[v][u]) for the four u: the min-plus step down an edge (sk_msg is the step up)
__device__ inline uint4 sksp_down(const SkCost& C, uint4 T) {
	return make_uint4(min(min(C.c[0] + T.x, C.c[4] + T.y), min(C.c[8] + T.z, C.c[12] + T.w)), min(min(C.c[1] + T.x, C.c[5] + T.y), min(C.c[9] + T.z, C.c[13] + T.w)),
	                  min(min(C.c[2] + T.x, C.c[6] + T.y), min(C.c[10] + T.z, C.c[14] + T.w)), min(min(C.c[3] + T.x, C.c[7] + T.y), min(C.c[11] + T.z, C.c[15] + T.w)));
}

// lst[0 .. n_lst): the batch's units (a unit: a lineage and a node c of it, unit_lin / unit_off as k_spr_score's) of this launch.  cap: the
// nodes the launch's LDS (and slab) is cut for.  IN_LDS: the slab is the head of the LDS and the sums follow it; otherwise the slab is
// slabs + blockIdx.x * cap * 64 and the LDS holds the sums alone.  key_d[unit], key_cy[unit]: written for every unit of an active
// lineage, SKSP_KEY_NONE where c is no pruned node or has no y
template <bool IN_LDS>
__global__ __launch_bounds__(64) void k_sksp_score(const u32* __restrict__ lst, u32 n_lst, const u32* __restrict__ unit_lin, const u32* __restrict__ unit_off,
                                                   const NjFit* __restrict__ fits, const char* __restrict__ contigs, const TreeRow* __restrict__ ri,
                                                   const u32* __restrict__ kid, const u32* __restrict__ par, const u32* __restrict__ leaf_par,
                                                   const u32* __restrict__ rootkid, const uint4* __restrict__ msg_all, const u32* __restrict__ active,
                                                   long long* __restrict__ key_d, u32* __restrict__ key_cy, ull* __restrict__ cands, uint4* __restrict__ slabs,
                                                   u32 cap, const SkCost C) {
	extern __shared__ uint4 sksp_lds[];
	uint4* slab = IN_LDS ? sksp_lds : slabs + (size_t) blockIdx.x * cap * 64u;
	ull* sums = (ull*) (IN_LDS ? sksp_lds + (size_t) cap * 64u : sksp_lds);
	const u32 lane = threadIdx.x;
	for (u32 i = blockIdx.x; i < n_lst; i += gridDim.x) {
		const u32 unit = lst[i], lin = unit_lin[unit];
		if (!active[lin]) continue;                          // (the whole wave)
		const NjFit q = fits[lin];
		const u32 m = q.m, nodes = 2u * m - 2u, c = unit - unit_off[lin], rk = rootkid[lin];
		if (c == q.root || c == rk) {
			if (lane == 0) { key_d[unit] = SKSP_KEY_NONE; key_cy[unit] = 0u; }
			continue;
		}
		const u32* K = kid + 2u * q.node0;                   // K[2 (v - m)], K[2 (v - m) + 1]
		const u32* U = par + q.node0;
		const u32 p = c < m ? leaf_par[q.first + c] : U[c - m];                      // (an inferred node: c is not the root's child)
		const u32 s = K[2u * (p - m)] == c ? K[2u * (p - m) + 1u] : K[2u * (p - m)], g = U[p - m];
		const u32 top = rk == p ? s : rk;                    // the root's child in T'
		__syncthreads();                                     // (the unit before has read its sums)
		for (u32 v = lane; v < nodes; v += 64u) sums[v] = SKSP_SUM_NONE;
		__syncthreads();
		u64 base = 0;                                        // the lane's share of W(T), all tiles
		u32 ncand = 0;
		for (u32 col0 = 0; col0 < q.w; col0 += 64u) {
			const bool live = col0 + lane < q.w, first = col0 == 0;
			const u32 cc = live ? col0 + lane : 0u;
			const uint4* H = msg_all + q.fs_off + cc;
			const u32 rb = sk_code(contigs[ri[q.first + q.root].at + cc]);
			// the tile's messages of every node into the slab: loads that do not wait for one another.  The walks below then read a
			// lane's own vectors only
#pragma unroll 4
			for (u32 v = 0; v < m; v++) slab[(size_t) v * 64u + lane] = sk_leaf_msg(C, sk_code(contigs[ri[q.first + v].at + cc]));
#pragma unroll 4
			for (u32 v = m; v < nodes; v++) slab[(size_t) v * 64u + lane] = H[(size_t) (v - m) * q.w];
			// msg_t(y) is valid until E'(y) is stored over the vector (below): every use comes before that store
			auto msg_t = [&](u32 y) { return slab[(size_t) y * 64u + lane]; };
			const uint4 Hc = msg_t(c);
			base += live ? (u64) sk_root_term(msg_t(rk), rb) : 0ull;                 // (rk is p or on the path: read before H' goes over it)
			// H' of the path from g up: s in p's place
			u32 prev = p;
			uint4 nw = msg_t(s);
			for (u32 x = g; x != q.root; x = U[x - m]) {
				nw = sk_msg(C, sk_add(nw, msg_t(K[2u * (x - m)] == prev ? K[2u * (x - m) + 1u] : K[2u * (x - m)])));
				slab[(size_t) x * 64u + lane] = nw;
				prev = x;
			}
			auto score = [&](u32 y, uint4 Hy, uint4 Ey) {        // (y, its vectors: wave-uniform y)
				if (y == s) return;                              // the edge above s is the old place
				const u32 mine = live ? sk_min(sk_add(sk_add(Ey, Hc), Hy)) : 0u;
				const u64 sum = vdjx_wave_sum64((u64) mine);   // (64 columns of a large lineage under large costs pass 2^32)
				if (lane == 0) sums[y] = first ? sum : sums[y] + sum;
				ncand += first ? 1u : 0u;
			};
			const uint4 Et = rb > 3u ? make_uint4(0u, 0u, 0u, 0u) : sk_row(C, rb);
			score(top, msg_t(top), Et);
			slab[(size_t) top * 64u + lane] = Et;
			u32 x = top;
			while (x >= m) {                                     // expand x: its children's E', their scores
				u32 a = K[2u * (x - m)], b = K[2u * (x - m) + 1u];
				a = a == p ? s : a;
				b = b == p ? s : b;
				const uint4 Ex = slab[(size_t) x * 64u + lane], Ha = msg_t(a), Hb = msg_t(b);
				const uint4 Ea = sksp_down(C, sk_add(Ex, Hb)), Eb = sksp_down(C, sk_add(Ex, Ha));
				score(a, Ha, Ea);
				score(b, Hb, Eb);
				slab[(size_t) a * 64u + lane] = Ea;              // (H' of a and b, read above, is not needed again)
				slab[(size_t) b * 64u + lane] = Eb;
				if (a >= m) { x = a; continue; }
				if (b >= m) { x = b; continue; }
				for (;;) {                                       // x is done: up, until a second child waits
					if (x == top) { x = 0u; break; }             // (a leaf id: the walk is over)
					u32 z = U[x - m];
					z = z == p ? g : z;
					u32 ka = K[2u * (z - m)], kb = K[2u * (z - m) + 1u];
					ka = ka == p ? s : ka;
					kb = kb == p ? s : kb;
					if (ka == x && kb >= m) { x = kb; break; }
					x = z;
				}
			}
		}
		__syncthreads();
		const long long total = (long long) vdjx_wave_sum64(base);
		long long best = SKSP_KEY_NONE;                      // the order of (delta, c, y); c is the unit's
		u32 best_y = 0xFFFFu;
		for (u32 v = lane; v < nodes; v += 64u) {
			const ull sv = sums[v];
			if (sv == SKSP_SUM_NONE) continue;
			const long long d = (long long) sv - total;
			if (d < best || (d == best && v < best_y)) { best = d; best_y = v; }
		}
#pragma unroll
		for (int off = 32; off >= 1; off >>= 1) {
			const long long t = (long long) vdjx_shfl_xor64((u64) best, off);
			const u32 ty = (u32) __shfl_xor((int) best_y, off, 64);
			if (t < best || (t == best && ty < best_y)) { best = t; best_y = ty; }
		}
		if (lane == 0) {
			key_d[unit] = best;
			key_cy[unit] = c << 16 | best_y;
			if (ncand) atomicAdd(cands + lin, (ull) ncand);
		}
	}
}

// one workgroup per searched lineage (which[]).  The messages above the pruned place are rewritten on the old kid / par; thread 0 rewires
// between two barriers; the messages from the regrafted place up are rewritten on the new ones.  A walk ends where a node's message comes
// out as stored: nothing above it changes
__global__ __launch_bounds__(SKSP_PICK_T) void k_sksp_pick(const u32* __restrict__ which, const NjFit* __restrict__ fits, const u32* __restrict__ unit_off,
                                                           const char* __restrict__ contigs, const TreeRow* __restrict__ ri, u32* kid, u32* par, u32* leaf_par,
                                                           u32* rootkid, uint4* msg_all, ull* W, u32* active, const long long* __restrict__ key_d,
                                                           const u32* __restrict__ key_cy, u32* moves, u32* rounds, u32* still, const SkCost C) {
	__shared__ long long wbest[SKSP_PICK_T / 64];
	__shared__ u32 wbest_cy[SKSP_PICK_T / 64];
	const u32 lin = which[blockIdx.x], tid = threadIdx.x;
	if (!active[lin]) return;                              // (the whole workgroup)
	const NjFit q = fits[lin];
	const u32 m = q.m, nodes = 2u * m - 2u;
	const long long* kd = key_d + unit_off[lin];
	const u32* kc = key_cy + unit_off[lin];
	long long best = SKSP_KEY_NONE;
	u32 low = 0xFFFFFFFFu;
	for (u32 i = tid; i < nodes; i += SKSP_PICK_T) {
		const long long d = kd[i];
		const u32 cy = kc[i];
		if (d < best || (d == best && cy < low)) { best = d; low = cy; }
	}
#pragma unroll
	for (int off = 32; off >= 1; off >>= 1) {
		const long long t = (long long) vdjx_shfl_xor64((u64) best, off);
		const u32 tc = (u32) __shfl_xor((int) low, off, 64);
		if (t < best || (t == best && tc < low)) { best = t; low = tc; }
	}
	if ((tid & 63u) == 0) { wbest[tid >> 6] = best; wbest_cy[tid >> 6] = low; }
	__syncthreads();
	best = wbest[0];
	low = wbest_cy[0];
	for (u32 w = 1; w < SKSP_PICK_T / 64; w++)
		if (wbest[w] < best || (wbest[w] == best && wbest_cy[w] < low)) { best = wbest[w]; low = wbest_cy[w]; }
	const long long d = best == SKSP_KEY_NONE ? 0ll : best;
	if (tid == 0) rounds[lin]++;
	if (d >= 0) {
		if (tid == 0) active[lin] = 0;
		return;
	}
	u32* K = kid + 2u * q.node0;
	u32* U = par + q.node0;
	const u32 c = low >> 16, y = low & 0xFFFFu;
	const u32 p = c < m ? leaf_par[q.first + c] : U[c - m], x = y < m ? leaf_par[q.first + y] : U[y - m];
	const u32 s = K[2u * (p - m)] == c ? K[2u * (p - m) + 1u] : K[2u * (p - m)], g = U[p - m];
	auto msg_of = [&](u32 v, u32 col) {
		return v < m ? sk_leaf_msg(C, sk_code(contigs[ri[q.first + v].at + col])) : msg_all[q.fs_off + (size_t) (v - m) * q.w + col];
	};
	for (u32 col = tid; col < q.w; col += SKSP_PICK_T) {  // s in p's place: the messages from g up
		uint4* H = msg_all + q.fs_off + col;
		u32 prev = p;
		uint4 nw = msg_of(s, col), old = msg_of(p, col);
		for (u32 z = g; z != q.root && sk_ne(nw, old); z = U[z - m]) {
			nw = sk_msg(C, sk_add(nw, msg_of(K[2u * (z - m)] == prev ? K[2u * (z - m) + 1u] : K[2u * (z - m)], col)));
			old = H[(size_t) (z - m) * q.w];
			H[(size_t) (z - m) * q.w] = nw;
			prev = z;
		}
	}
	__syncthreads();
	if (tid == 0) {
		auto set_parent = [&](u32 v, u32 to) { if (v < m) leaf_par[q.first + v] = to; else U[v - m] = to; };
		auto replace_kid = [&](u32 z, u32 from, u32 to) {
			if (z == q.root) { rootkid[lin] = to; return; }
			u32* k = K + 2u * (z - m);
			const u32 other = k[0] == from ? k[1] : k[0];
			k[0] = min(other, to);
			k[1] = max(other, to);
		};
		replace_kid(g, p, s);
		set_parent(s, g);
		replace_kid(x, y, p);
		set_parent(p, x);
		K[2u * (p - m)] = min(c, y);
		K[2u * (p - m) + 1u] = max(c, y);
		set_parent(y, p);
		W[lin] = (ull) ((long long) W[lin] + d);
		moves[lin]++;
		atomicAdd(still, 1u);
	}
	__syncthreads();
	for (u32 col = tid; col < q.w; col += SKSP_PICK_T) {  // p above y: the messages from p up
		uint4* H = msg_all + q.fs_off + col;
		u32 prev = p;
		uint4 nw = sk_msg(C, sk_add(msg_of(c, col), msg_of(y, col)));
		H[(size_t) (p - m) * q.w] = nw;
		for (u32 z = x; z != q.root; z = U[z - m]) {
			nw = sk_msg(C, sk_add(nw, msg_of(K[2u * (z - m)] == prev ? K[2u * (z - m) + 1u] : K[2u * (z - m)], col)));
			if (!sk_ne(nw, H[(size_t) (z - m) * q.w])) break;
			H[(size_t) (z - m) * q.w] = nw;
			prev = z;
		}
	}
}

extern "C" int vdjx_tree_sankoff_spr(vdjx_ctx* c, const char* contigs, size_t n, int len, const int32_t* clone, const int32_t* anchor, const uint32_t* prio,
                                     const uint32_t* cost, const int32_t* start_parent, const vdjx_tree_sankoff_spr_params* params, int32_t* out_parent,
                                     int64_t* out_cost, int32_t* out_mutations, int32_t* out_depth, int32_t* out_clone, char* out_anc,
                                     vdjx_tree_sankoff_info* info) {
	static const char* who = "vdjx_tree_sankoff_spr";
	if (info) memset(info, 0, sizeof *info);
	if (!c) { vdjx_set_error("%s: NULL argument", who); return VDJX_EINVAL; }
	if (params && (params->reserved[0] || params->reserved[1] || params->reserved[2])) {
		vdjx_set_error("%s: params.reserved is {%u, %u, %u} (it must be 0)", who, params->reserved[0], params->reserved[1], params->reserved[2]);
		return VDJX_EINVAL;
	}
	SkCost C;
	if (cost) memcpy(C.c, cost, sizeof C.c); else sk_unit_costs(C.c);
	if (const int bad = sk_check_costs(C.c); bad >= 0) {
		vdjx_set_error("%s: cost[%d][%d] is %u (%s)", who, bad >> 2, bad & 3, C.c[bad], (bad >> 2) == (bad & 3) ? "the diagonal is 0" : "an off-diagonal cell is 1 .. 65535");
		return VDJX_EINVAL;
	}
	if (n == 0) return VDJX_OK;
	if (!contigs || !clone || !anchor || !out_parent || !out_cost || !out_mutations || !out_depth || !out_clone) {
		vdjx_set_error("%s: NULL argument", who);
		return VDJX_EINVAL;
	}
	if (int rc = tree_check_contigs(who, contigs, n, len)) return rc;
	const auto t0 = std::chrono::steady_clock::now();       // (where vdjx_tree_mp starts its clock)
	const u32 max_rounds = params ? params->max_rounds : 0u;
	std::vector<u64> keys;
	if (int rc = tree_keys(who, n, len, clone, anchor, keys)) return rc;
	const u32 rows = (u32) keys.size();
	TreeLay L;
	if (rows)
		if (int rc = tree_lay(who, keys, len, clone, anchor, prio, L)) return rc;
	vdjx_tree_sankoff_info inf;
	memset(&inf, 0, sizeof inf);
	inf.members = rows;
	inf.clones = (u32) L.clones.size();
	inf.largest_clone = L.largest;
	std::vector<u32> big, size;                            // the lineages of two and more: their index in L.clones, their members
	std::vector<u64> inf0(L.clones.size());                // per lineage: its first inferred node among the call's
	for (size_t k = 0; k < L.clones.size(); k++) {
		const TreeClone& q = L.clones[k];
		if (q.m > VDJX_SPR_MAX_MEMBERS) {
			vdjx_set_error("%s: clone %d has %u members (at most %u)", who, clone[L.row_item[q.first]], q.m, VDJX_SPR_MAX_MEMBERS);
			return VDJX_ELIMIT;
		}
		inf0[k] = inf.internal;
		if (q.m >= 2) { big.push_back((u32) k); size.push_back(q.m); inf.edges += 2ull * q.m - 3; }
		if (q.m >= 3) inf.internal += q.m - 2;
		if (q.m >= 4) inf.searched++;
	}
	const u64 nodes = (u64) n + inf.internal;
	// the start: the caller's parents, or vdjx_tree_nj's for the same arguments (vdjx_nj_parents); every lineage's parents are checked
	// before this call's own GPU work, as vdjx_tree_mp checks them
	std::vector<int32_t> nj_parent;
	if (!start_parent && !big.empty()) {
		nj_parent.resize((size_t) nodes);
		if (int rc = vdjx_nj_parents(c, contigs, n, len, clone, anchor, prio, nj_parent.data())) return rc;
	}
	const int32_t* start = start_parent ? start_parent : nj_parent.data();
	std::vector<int32_t> item_row(n, -1), lp;              // lp: the local parents of every lineage's nodes, lineage after lineage
	std::vector<u64> lp_off(L.clones.size()), cand0(L.clones.size(), 0);      // cand0: the candidates of the start tree's round
	for (u32 r = 0; r < rows; r++) item_row[L.row_item[r]] = (int32_t) r;
	NjTree t;
	for (size_t k = 0; k < L.clones.size(); k++) {
		const TreeClone& q = L.clones[k];
		const u32 m = q.m, nl = m < 3 ? m : 2 * m - 2;
		lp_off[k] = lp.size();
		for (u32 v = 0; v < nl; v++) {
			const u64 s = v < m ? (u64) L.row_item[q.first + v] : (u64) n + inf0[k] + (v - m);
			lp.push_back(q.first + v == q.root ? -1 : mp_local(start[s], n, item_row.data(), q.first, m, inf0[k]));
		}
		if (const int e = mp_orient(m, q.root - q.first, lp.data() + lp_off[k], t)) {
			vdjx_set_error("%s: %s of clone %d (%u members) are no tree: %s", who, start_parent ? "the start parents" : "vdjx_tree_nj's parents",
			               clone[L.row_item[q.first]], m, mp_why(e));
			return start_parent ? VDJX_EINVAL : VDJX_ESTATE;
		}
		cand0[k] = spr_candidates(m, q.root - q.first, t);
	}
	for (u64 s = 0; s < nodes; s++) { out_parent[s] = out_mutations[s] = out_depth[s] = out_clone[s] = -1; out_cost[s] = -1; }
	if (out_anc) memset(out_anc, 0, (size_t) inf.internal * (size_t) len);
	for (const TreeClone& q : L.clones)
		if (q.m == 1) {                                       // a lone root
			const u32 i = L.row_item[q.first];
			out_depth[i] = 0;
			out_clone[i] = clone[i];
		}
	std::vector<u32> end;
	const u64 knob = (u64) vdjx_env_num("VDJX_NJ_CELLS", 1ll << 26, 1, 1ll << 28);
	link_batches(size, knob, end);
	inf.batches = (u32) end.size();
	u64 w_final = 0;
	if (!big.empty()) {
		HIP_TRY(hipSetDevice(c->device));
		hipStream_t st = c->stream;
		vdjx_work wk(c);
		char *d_contigs, *d_anc = nullptr;
		TreeRow* d_ri;
		u32 *d_mut_row, *d_mut_inf, *d_leaf_par, *d_still;
		ull *d_cost_row, *d_cost_inf;
		HIP_TRY(wk.alloc(&d_contigs, n * (size_t) len));
		HIP_TRY(wk.alloc(&d_ri, (size_t) rows + 1));
		HIP_TRY(wk.alloc(&d_mut_row, rows));
		HIP_TRY(wk.alloc(&d_mut_inf, inf.internal));
		HIP_TRY(wk.alloc(&d_cost_row, rows));
		HIP_TRY(wk.alloc(&d_cost_inf, inf.internal));
		HIP_TRY(wk.alloc(&d_leaf_par, rows));
		HIP_TRY(wk.alloc(&d_still, 1));
		if (out_anc && inf.internal) {
			HIP_TRY(wk.alloc(&d_anc, (size_t) inf.internal * (size_t) len));
			HIP_TRY(hipMemsetAsync(d_anc, 0, (size_t) inf.internal * (size_t) len, st));
		}
		HIP_TRY(hipMemcpyAsync(d_contigs, contigs, n * (size_t) len, hipMemcpyHostToDevice, st));
		HIP_TRY(hipMemcpyAsync(d_ri, L.ri.data(), ((size_t) rows + 1) * sizeof(TreeRow), hipMemcpyHostToDevice, st));
		HIP_TRY(hipMemsetAsync(d_mut_row, 0, (size_t) rows * sizeof(u32), st));
		HIP_TRY(hipMemsetAsync(d_mut_inf, 0, (size_t) (inf.internal ? inf.internal : 1) * sizeof(u32), st));
		HIP_TRY(hipMemsetAsync(d_cost_row, 0, (size_t) rows * sizeof(ull), st));
		HIP_TRY(hipMemsetAsync(d_cost_inf, 0, (size_t) (inf.internal ? inf.internal : 1) * sizeof(ull), st));
		const vdjx_arena::mark_t mk = wk.mark();
		std::vector<u32> h_kid, h_par, h_order, leaf_par(rows, 0u), unit_lin, unit_off, lst_8, lst_2, lst_slab, which, ones, h_rootkid, h_moves, h_rounds;
		std::vector<ull> h_W, h_W0, h_cands;
		std::vector<NjFit> fits;
		std::vector<NjFitItem> fit_items;
		volatile u32* h_still = (volatile u32*) (u32*) c->h_pin;
		for (size_t b = 0, k0 = 0; b < end.size(); k0 = end[b++]) {
			const size_t k1 = end[b], nl = k1 - k0;
			fits.clear(); fit_items.clear(); h_kid.clear(); h_par.clear(); h_order.clear(); which.clear(); h_rootkid.clear();
			unit_lin.clear(); unit_off.assign(1, 0u); lst_8.clear(); lst_2.clear(); lst_slab.clear();
			u64 fs_cells = 0;
			u32 m_8 = 0, m_2 = 0, m_slab = 0;                    // the largest searched lineage of either LDS geometry and beyond the bound
			const u64 batch_inf0 = inf0[big[k0]];                // the batch's inferred nodes are a run of the call's
			const u32 row0 = L.clones[big[k0]].first, row1 = L.clones[big[k1 - 1]].first + L.clones[big[k1 - 1]].m;
			for (size_t k = k0; k < k1; k++) {
				const TreeClone& q = L.clones[big[k]];
				const u32 m = q.m, root = q.root - q.first;
				if (mp_orient(m, root, lp.data() + lp_off[big[k]], t)) { vdjx_set_error("%s: a checked tree is no tree any more", who); return VDJX_ESTATE; }
				for (u32 v = 0; v < (u32) t.parent.size(); v++) {
					if (t.parent[v] < 0) continue;
					if (v < m) leaf_par[q.first + v] = (u32) t.parent[v];
					else h_par.push_back((u32) t.parent[v]);    // (v ascends: index node0 + v - m)
				}
				h_kid.insert(h_kid.end(), t.kid.begin(), t.kid.end());
				h_rootkid.push_back(t.root_kid);
				fits.push_back({fs_cells, q.first, m, q.w, (u32) (inf0[big[k]] - batch_inf0), root, t.root_kid, (u32) h_order.size(), 0u});
				h_order.insert(h_order.end(), t.order.begin(), t.order.end());
				for (u32 c0 = 0; c0 < q.w; c0 += 64u) fit_items.push_back({(u32) (k - k0), c0});
				const u32 nu = m > 3 ? 2u * m - 2u : 0u;          // a unit per node: the root leaf's and its child's write an empty key
				std::vector<u32>& lst = m <= SKSP_LDS_MEMBERS_8 ? lst_8 : m <= VDJX_SKSP_LDS_MEMBERS ? lst_2 : lst_slab;
				for (u32 v = 0; v < nu; v++) lst.push_back(unit_off.back() + v);
				unit_lin.insert(unit_lin.end(), nu, (u32) (k - k0));
				unit_off.push_back(unit_off.back() + nu);
				if (nu) {
					which.push_back((u32) (k - k0));
					u32& top = m <= SKSP_LDS_MEMBERS_8 ? m_8 : m <= VDJX_SKSP_LDS_MEMBERS ? m_2 : m_slab;
					top = std::max(top, m);
				}
				fs_cells += (u64) (m - 2u) * q.w;
			}
			const u32 n_unit = unit_off.back();                  // (below 2^21: a call has fewer than 2^20 items)
			auto nodes_of = [](u32 m) { return m ? 2u * m - 2u : 0u; };
			const u32 cap_8 = nodes_of(m_8), cap_2 = nodes_of(m_2), cap_slab = nodes_of(m_slab);
			const u32 grid_slab = std::min((u32) lst_slab.size(), SKSP_SLAB_WGS);
			ones.assign(nl, 0u);
			for (u32 l : which) ones[l] = 1u;
			NjFit* d_fits;
			NjFitItem* d_fit_items;
			u32 *d_kid, *d_par, *d_order, *d_unit_lin, *d_unit_off, *d_lst_8, *d_lst_2, *d_lst_slab, *d_which, *d_rootkid, *d_active, *d_moves, *d_rounds, *d_key_cy;
			long long* d_key_d;
			ull *d_cands, *d_W;
			uint4 *d_msg, *d_slabs;
			uint8_t* d_state;
			HIP_TRY(wk.alloc(&d_fits, nl));
			HIP_TRY(wk.alloc(&d_fit_items, fit_items.size()));
			HIP_TRY(wk.alloc(&d_kid, h_kid.size()));
			HIP_TRY(wk.alloc(&d_par, h_par.size()));
			HIP_TRY(wk.alloc(&d_order, h_order.size()));
			HIP_TRY(wk.alloc(&d_unit_lin, n_unit));
			HIP_TRY(wk.alloc(&d_unit_off, nl + 1));
			HIP_TRY(wk.alloc(&d_lst_8, lst_8.size()));
			HIP_TRY(wk.alloc(&d_lst_2, lst_2.size()));
			HIP_TRY(wk.alloc(&d_lst_slab, lst_slab.size()));
			HIP_TRY(wk.alloc(&d_which, which.size()));
			HIP_TRY(wk.alloc(&d_rootkid, nl));
			HIP_TRY(wk.alloc(&d_W, nl));
			HIP_TRY(wk.alloc(&d_active, nl));
			HIP_TRY(wk.alloc(&d_moves, nl));
			HIP_TRY(wk.alloc(&d_rounds, nl));
			HIP_TRY(wk.alloc(&d_key_d, n_unit));
			HIP_TRY(wk.alloc(&d_key_cy, n_unit));
			HIP_TRY(wk.alloc(&d_cands, nl));
			HIP_TRY(wk.alloc(&d_msg, (size_t) fs_cells));
			HIP_TRY(wk.alloc(&d_state, (size_t) fs_cells));
			HIP_TRY(wk.alloc(&d_slabs, (size_t) grid_slab * cap_slab * 64u));
			HIP_TRY(hipMemcpyAsync(d_fits, fits.data(), nl * sizeof(NjFit), hipMemcpyHostToDevice, st));
			HIP_TRY(hipMemcpyAsync(d_fit_items, fit_items.data(), fit_items.size() * sizeof(NjFitItem), hipMemcpyHostToDevice, st));
			if (!h_kid.empty()) {
				HIP_TRY(hipMemcpyAsync(d_kid, h_kid.data(), h_kid.size() * sizeof(u32), hipMemcpyHostToDevice, st));
				HIP_TRY(hipMemcpyAsync(d_par, h_par.data(), h_par.size() * sizeof(u32), hipMemcpyHostToDevice, st));
				HIP_TRY(hipMemcpyAsync(d_order, h_order.data(), h_order.size() * sizeof(u32), hipMemcpyHostToDevice, st));
			}
			HIP_TRY(hipMemcpyAsync(d_leaf_par + row0, leaf_par.data() + row0, (size_t) (row1 - row0) * sizeof(u32), hipMemcpyHostToDevice, st));
			if (n_unit) HIP_TRY(hipMemcpyAsync(d_unit_lin, unit_lin.data(), (size_t) n_unit * sizeof(u32), hipMemcpyHostToDevice, st));
			HIP_TRY(hipMemcpyAsync(d_unit_off, unit_off.data(), (nl + 1) * sizeof(u32), hipMemcpyHostToDevice, st));
			if (!lst_8.empty()) HIP_TRY(hipMemcpyAsync(d_lst_8, lst_8.data(), lst_8.size() * sizeof(u32), hipMemcpyHostToDevice, st));
			if (!lst_2.empty()) HIP_TRY(hipMemcpyAsync(d_lst_2, lst_2.data(), lst_2.size() * sizeof(u32), hipMemcpyHostToDevice, st));
			if (!lst_slab.empty()) HIP_TRY(hipMemcpyAsync(d_lst_slab, lst_slab.data(), lst_slab.size() * sizeof(u32), hipMemcpyHostToDevice, st));
			if (!which.empty()) HIP_TRY(hipMemcpyAsync(d_which, which.data(), which.size() * sizeof(u32), hipMemcpyHostToDevice, st));
			HIP_TRY(hipMemcpyAsync(d_rootkid, h_rootkid.data(), nl * sizeof(u32), hipMemcpyHostToDevice, st));
			HIP_TRY(hipMemcpyAsync(d_active, ones.data(), nl * sizeof(u32), hipMemcpyHostToDevice, st));
			HIP_TRY(hipMemsetAsync(d_W, 0, nl * sizeof(ull), st));
			HIP_TRY(hipMemsetAsync(d_moves, 0, nl * sizeof(u32), st));
			HIP_TRY(hipMemsetAsync(d_rounds, 0, nl * sizeof(u32), st));
			HIP_TRY(hipMemsetAsync(d_cands, 0, nl * sizeof(ull), st));
			{
				vdjx_prof_scope ps(c, "k_sk_up");
				hipLaunchKernelGGL(k_sk_up, dim3((u32) fit_items.size()), dim3(64), 0, st, (const NjFitItem*) d_fit_items, (const NjFit*) d_fits, (const char*) d_contigs,
				                   (const TreeRow*) d_ri, (const u32*) d_kid, (const u32*) d_order, d_msg, d_W, C);
			}
			h_W0.resize(nl); h_W.resize(nl); h_moves.resize(nl); h_rounds.resize(nl); h_cands.resize(nl);
			HIP_TRY(hipMemcpyAsync(h_W0.data(), d_W, nl * sizeof(ull), hipMemcpyDeviceToHost, st));
			HIP_TRY(hipStreamSynchronize(st));                  // (the host vectors above are free again; so is h_pin's first word)
			auto score = [&](auto kernel, const char* name, const u32* d_lst, u32 n_lst, u32 grid, u32 lds, uint4* slabs, u32 cap) {
				vdjx_prof_scope ps(c, name);
				hipLaunchKernelGGL(kernel, dim3(grid), dim3(64), lds, st, d_lst, n_lst, (const u32*) d_unit_lin, (const u32*) d_unit_off, (const NjFit*) d_fits,
				                   (const char*) d_contigs, (const TreeRow*) d_ri, (const u32*) d_kid, (const u32*) d_par, (const u32*) d_leaf_par,
				                   (const u32*) d_rootkid, (const uint4*) d_msg, (const u32*) d_active, d_key_d, d_key_cy, d_cands, slabs, cap, C);
			};
			for (u32 round = 1; n_unit; round++) {
				HIP_TRY(hipMemsetAsync(d_still, 0, sizeof(u32), st));
				if (!lst_8.empty())
					score(k_sksp_score<true>, "k_sksp_score", d_lst_8, (u32) lst_8.size(), (u32) lst_8.size(), cap_8 * SKSP_NODE_LDS_BYTES, nullptr, cap_8);
				if (!lst_2.empty())
					score(k_sksp_score<true>, "k_sksp_score", d_lst_2, (u32) lst_2.size(), (u32) lst_2.size(), cap_2 * SKSP_NODE_LDS_BYTES, nullptr, cap_2);
				if (!lst_slab.empty())
					score(k_sksp_score<false>, "k_sksp_score_slab", d_lst_slab, (u32) lst_slab.size(), grid_slab, cap_slab * (SKSP_NODE_LDS_BYTES - 1024u), d_slabs, cap_slab);
				{
					vdjx_prof_scope ps(c, "k_sksp_pick");
					hipLaunchKernelGGL(k_sksp_pick, dim3((u32) which.size()), dim3(SKSP_PICK_T), 0, st, (const u32*) d_which, (const NjFit*) d_fits, (const u32*) d_unit_off,
					                   (const char*) d_contigs, (const TreeRow*) d_ri, d_kid, d_par, d_leaf_par, d_rootkid, d_msg, d_W, d_active,
					                   (const long long*) d_key_d, (const u32*) d_key_cy, d_moves, d_rounds, d_still, C);
				}
				HIP_TRY(hipMemcpyAsync((void*) h_still, d_still, sizeof(u32), hipMemcpyDeviceToHost, st));
				HIP_TRY(hipStreamSynchronize(st));
				HIP_TRY(hipGetLastError());
				if (*h_still == 0 || round == max_rounds) break;
			}
			// the host's part: root every lineage's final parents, fill the outputs that need no sequence, give the down pass its order
			HIP_TRY(hipMemcpyAsync(h_W.data(), d_W, nl * sizeof(ull), hipMemcpyDeviceToHost, st));
			HIP_TRY(hipMemcpyAsync(h_moves.data(), d_moves, nl * sizeof(u32), hipMemcpyDeviceToHost, st));
			HIP_TRY(hipMemcpyAsync(h_rounds.data(), d_rounds, nl * sizeof(u32), hipMemcpyDeviceToHost, st));
			HIP_TRY(hipMemcpyAsync(h_cands.data(), d_cands, nl * sizeof(ull), hipMemcpyDeviceToHost, st));
			if (!h_par.empty()) HIP_TRY(hipMemcpyAsync(h_par.data(), d_par, h_par.size() * sizeof(u32), hipMemcpyDeviceToHost, st));
			HIP_TRY(hipMemcpyAsync(leaf_par.data() + row0, d_leaf_par + row0, (size_t) (row1 - row0) * sizeof(u32), hipMemcpyDeviceToHost, st));
			HIP_TRY(hipStreamSynchronize(st));
			h_order.clear();
			std::vector<int32_t> fp;
			for (size_t k = k0; k < k1; k++) {
				const TreeClone& q = L.clones[big[k]];
				NjFit& f = fits[k - k0];
				const u32 m = q.m, root = f.root;
				fp.assign(m < 3 ? m : 2 * m - 2, -1);
				for (u32 v = 0; v < (u32) fp.size(); v++)
					if (v != root) fp[v] = (int32_t) (v < m ? leaf_par[q.first + v] : h_par[f.node0 + v - m]);
				if (const int e = mp_orient(m, root, fp.data(), t)) {
					vdjx_set_error("%s: the searched parents of clone %d (%u members) are no tree: %s", who, clone[L.row_item[q.first]], m, mp_why(e));
					return VDJX_ESTATE;
				}
				if (h_rounds[k - k0] == 1 && h_cands[k - k0] != cand0[big[k]]) {
					vdjx_set_error("%s: clone %d's first round scored %llu candidates, its start tree has %llu", who, clone[L.row_item[q.first]],
					               h_cands[k - k0], (ull) cand0[big[k]]);
					return VDJX_ESTATE;
				}
				f.root_kid = t.root_kid;                           // (a move can change the root's child: the down pass reads it here)
				const u64 a0 = inf0[big[k]];
				auto slot = [&](u32 v) { return v < m ? (u64) L.row_item[q.first + v] : (u64) n + a0 + (v - m); };
				for (u32 v = 0; v < (u32) t.parent.size(); v++) {
					const u64 s = slot(v);
					out_clone[s] = clone[L.row_item[q.first]];
					out_depth[s] = t.depth[v];
					out_parent[s] = t.parent[v] < 0 ? -1 : (int32_t) slot((u32) t.parent[v]);
				}
				h_order.insert(h_order.end(), t.order.begin(), t.order.end());
				inf.cost_start += h_W0[k - k0];
				w_final += h_W[k - k0];
				inf.moves += h_moves[k - k0];
				inf.moved += h_moves[k - k0] > 0;
				inf.rounds = std::max(inf.rounds, h_rounds[k - k0]);
				inf.candidates += h_cands[k - k0];
			}
			if (!h_order.empty()) HIP_TRY(hipMemcpyAsync(d_order, h_order.data(), h_order.size() * sizeof(u32), hipMemcpyHostToDevice, st));
			HIP_TRY(hipMemcpyAsync(d_fits, fits.data(), nl * sizeof(NjFit), hipMemcpyHostToDevice, st));
			{
				vdjx_prof_scope ps(c, "k_sk_down");
				hipLaunchKernelGGL(k_sk_down, dim3((u32) fit_items.size()), dim3(64), 0, st, (const NjFitItem*) d_fit_items, (const NjFit*) d_fits, (const char*) d_contigs,
				                   (const TreeRow*) d_ri, (const u32*) d_kid, (const u32*) d_par, (const u32*) d_order, (const u32*) d_leaf_par, (const uint4*) d_msg,
				                   d_state, d_cost_row, d_cost_inf + batch_inf0, d_mut_row, d_mut_inf + batch_inf0,
				                   d_anc ? d_anc + (size_t) batch_inf0 * (size_t) len : nullptr, (u32) len, C);
			}
			HIP_TRY(hipStreamSynchronize(st));                  // (the host vectors are uploaded from again, and the workspace is given up)
			HIP_TRY(hipGetLastError());
			vdjx_prof_collect(c, false);
			wk.release_to(mk);
		}
		std::vector<u32> mut_row(rows), mut_inf((size_t) inf.internal);
		std::vector<ull> cost_row(rows), cost_inf((size_t) inf.internal);
		HIP_TRY(hipMemcpyAsync(mut_row.data(), d_mut_row, (size_t) rows * sizeof(u32), hipMemcpyDeviceToHost, st));
		HIP_TRY(hipMemcpyAsync(cost_row.data(), d_cost_row, (size_t) rows * sizeof(ull), hipMemcpyDeviceToHost, st));
		if (inf.internal) {
			HIP_TRY(hipMemcpyAsync(mut_inf.data(), d_mut_inf, (size_t) inf.internal * sizeof(u32), hipMemcpyDeviceToHost, st));
			HIP_TRY(hipMemcpyAsync(cost_inf.data(), d_cost_inf, (size_t) inf.internal * sizeof(ull), hipMemcpyDeviceToHost, st));
		}
		if (d_anc) HIP_TRY(hipMemcpyAsync(out_anc, d_anc, (size_t) inf.internal * (size_t) len, hipMemcpyDeviceToHost, st));
		HIP_TRY(hipStreamSynchronize(st));
		for (u32 r = 0; r < rows; r++) {
			const u32 i = L.row_item[r];
			if (out_parent[i] < 0) continue;
			out_mutations[i] = (int32_t) mut_row[r];
			out_cost[i] = (int64_t) cost_row[r];
			inf.mutations += mut_row[r];
			inf.cost += cost_row[r];
		}
		for (u64 a = 0; a < inf.internal; a++) {
			out_mutations[n + a] = (int32_t) mut_inf[a];
			out_cost[n + a] = (int64_t) cost_inf[a];
			inf.mutations += mut_inf[a];
			inf.cost += cost_inf[a];
		}
		if (inf.cost != w_final) {
			vdjx_set_error("%s: the search ended at a cost of %llu, the final trees' edges cost %llu", who, (ull) w_final, (ull) inf.cost);
			return VDJX_ESTATE;
		}
	}
	if (info) *info = inf;
	c->stats["tree_sankoff_spr_candidates"] = inf.candidates;
	c->stats["tree_sankoff_spr_us"] = (u64) std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
	return VDJX_OK;
}
