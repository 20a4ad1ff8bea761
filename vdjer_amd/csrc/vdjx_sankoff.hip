// vdjx_sankoff.hip -- weighted (Sankoff) parsimony for the lineage trees: vdjx_tree_mp under a 4 x 4 cost matrix (gfx950 only, wave64).
//
//   vdjx_tree_sankoff   per lineage: from vdjx_tree_nj's tree or the caller's, the weighted cost W(T) of the rooted tree under cost[16],
//                       optionally vdjx_tree_mp's rounds of nearest-neighbour interchanges under the key (W, v, k), then the down pass:
//                       every inferred node's states, every edge's cost and mutations (the model: include/vdjx.h; in Python:
//                       tests/tree_sankoff_model.py)
//   vdjx_sankoff_costs  plain C, no GPU: a targeting model's 5-mer weights -> such a matrix (vdjx_sankoff_host.h)
//
// Everything around the score is vdjx_tree_mp's (vdjx_mp.hip): the layout (vdjx_treelay.h), the start's check (vdjx_mp_host.h), the
// batches, kid[2] and par of every inferred node, the parent of every leaf.  Where that call keeps one set byte per (inferred node,
// column), this one keeps the node's MESSAGE to its parent: H_x(s) = min_t (c[s][t] + S_x[t]) for the four parent states s -- one 16-byte
// vector of four uint32, the column the fastest index, so a lane's access is one 16-byte load or store and a wave's 1 KiB contiguous.
// Keeping H and not S makes a step of a walk one min-plus product: the parent's S is the stored vector of the other child plus the new
// one.  A leaf's message is a column of the matrix (or 0 for a wildcard) and is made from its character, never stored.  The sixteen costs
// are a kernel argument by value: uniform, in scalar registers; the 4 x 4 min-plus is unrolled.
//   k_sk_up        (vdjx_sankoff_dev.h, shared with vdjx_sankoff_spr.hip, as are the messages' helpers) one wave per (lineage, 64 columns), a
//                  lane per column: the messages in the host's post-order of the start tree, and W by one 64-bit integer atomicAdd per wave
//   k_sk_score     one wave per (lineage, candidate) and column tile, or over several tiles in turn (k_mp_score's grid).  A swap at (v, k)
//                  changes only the messages of v, p and p's ancestors: every lane recomputes v' and p' and walks towards the root against
//                  the STORED messages of the other children.  The cost only shows at the root: the lane's delta is the new root term less
//                  the stored one.  A ballot that says no lane's message differs from the stored one ends the walk early with a delta of 0
//                  (rare under unequal costs, common under unit costs on conserved columns).  The wave's sum goes into the candidate's
//                  int64 by an integer atomicAdd (a sum: any order)
//   k_sk_pick      one workgroup per lineage that is still searching: the smallest (delta, candidate); if the delta is negative one thread
//                  rewires kid and par, all threads rewrite the stored messages along the same path for every column, W follows
//   k_sk_down      (vdjx_sankoff_dev.h) one wave per (lineage, 64 columns), parents before children in the host's order of the final tree: the states (a byte
//                  per inferred node and column), the ancestors' characters, and per edge its cost (64-bit) and mutations by one integer
//                  atomicAdd per (node, wave) of wave-reduced sums
// The host reads one counter per round (page-locked) and stops at 0 or at max_rounds.  No floating point on the device, no spin-wait;
// nothing waits for another workgroup.  Scratch comes from the context's workspace.
#include "vdjx_common.h"
#include "vdjx_fitch.h"
#include "vdjx_link.h"
#include "vdjx_mp_host.h"
#include "vdjx_sankoff_dev.h"
#include "vdjx_sankoff_host.h"
#include "vdjx_treelay.h"

#include <string.h>

static_assert(VDJX_MP_MAX_MEMBERS == NJ_MAX_M, "the header's limit");
#define SK_STEP_SLOTS 64u                // the step counter is spread over this many words
#define SK_FILL_WAVES 16384u             // 256 CUs x 4 SIMDs x 16 waves
#define SK_PICK_T 256
#define SK_KEY_NONE 0x7FFFFFFFFFFFFFFFll
#define SK_KEY_CAND 65536ll              // key = delta * SK_KEY_CAND + candidate: a lineage has fewer than 8,192 candidates, |delta| < 2^43

// the j-th candidate node of a lineage: the inferred nodes but the root's child, ascending (vdjx_tree_mp's numbering)
__device__ inline u32 sk_cand_node(u32 m, u32 root_kid, u32 j) { return m + j + (m + j >= root_kid ? 1u : 0u); }

// blockIdx.x: a candidate of the batch, cand_lin[] its lineage, cand_off[nl + 1] the candidates of the lineages before.  The wave takes the
// column tiles blockIdx.y, blockIdx.y + gridDim.y, ...
__global__ __launch_bounds__(64) void k_sk_score(const NjFit* __restrict__ fits, const u32* __restrict__ cand_lin, const u32* __restrict__ cand_off,
                                                 const char* __restrict__ contigs, const TreeRow* __restrict__ ri, const u32* __restrict__ kid,
                                                 const u32* __restrict__ par, const uint4* __restrict__ msg_all, const u32* __restrict__ active,
                                                 ull* __restrict__ delta, ull* __restrict__ steps, const SkCost C) {
	const u32 lin = cand_lin[blockIdx.x], lane = threadIdx.x;
	if (!active[lin]) return;
	const NjFit q = fits[lin];
	const u32 m = q.m, cand = blockIdx.x - cand_off[lin];
	if (blockIdx.y * 64u >= q.w) return;
	const u32* K = kid + 2u * q.node0;                     // K[2 (v - m)], K[2 (v - m) + 1]
	const u32* U = par + q.node0;
	const u32 k = cand & 1u, v = sk_cand_node(m, q.root_kid, cand >> 1), p = U[v - m];
	const u32 s = K[2u * (p - m)] == v ? K[2u * (p - m) + 1u] : K[2u * (p - m)], c = K[2u * (v - m) + k], o = K[2u * (v - m) + 1u - k];
	long long d = 0;
	u32 made = 0;
	for (u32 col0 = blockIdx.y * 64u; col0 < q.w; col0 += gridDim.y * 64u) {
		const bool live = col0 + lane < q.w;
		const u32 cc = live ? col0 + lane : 0u;
		const uint4* H = msg_all + q.fs_off + cc;
		auto code = [&](u32 y) { return sk_code(contigs[ri[q.first + y].at + cc]); };
		auto msg_of = [&](u32 y) { return y < m ? sk_leaf_msg(C, code(y)) : H[(size_t) (y - m) * q.w]; };
		uint4 nw = sk_msg(C, sk_add(msg_of(c), sk_msg(C, sk_add(msg_of(s), msg_of(o)))));      // p's new message over v's new one
		uint4 old = H[(size_t) (p - m) * q.w];
		u32 x = p;
		long long dt = 0;
		made += 2u;
		while (__ballot(live && sk_ne(nw, old))) {
			const u32 g = U[x - m];
			if (g == q.root) {
				const u32 rb = code(g);
				dt = (long long) sk_root_term(nw, rb) - (long long) sk_root_term(old, rb);
				break;
			}
			nw = sk_msg(C, sk_add(nw, msg_of(K[2u * (g - m)] == x ? K[2u * (g - m) + 1u] : K[2u * (g - m)])));
			old = H[(size_t) (g - m) * q.w];
			x = g;
			made++;
		}
		d += live ? dt : 0ll;
	}
	d = (long long) vdjx_wave_sum64((u64) d);
	if (lane == 0) {
		if (d) atomicAdd(delta + blockIdx.x, (ull) d);
		atomicAdd(steps + ((blockIdx.x + blockIdx.y) % SK_STEP_SLOTS), (ull) made);
	}
}

// one workgroup per searched lineage (which[]).  kid, par and leaf_par are rewritten by thread 0 AFTER every thread has read the candidate's
// neighbourhood; what the threads read on their way up afterwards (par of p and above, kid above p) is nothing the move touches
__global__ __launch_bounds__(SK_PICK_T) void k_sk_pick(const u32* __restrict__ which, const NjFit* __restrict__ fits, const u32* __restrict__ cand_off,
                                                       const char* __restrict__ contigs, const TreeRow* __restrict__ ri, u32* kid, u32* par, u32* leaf_par,
                                                       uint4* msg_all, ull* W, u32* active, ull* delta, u32* moves, u32* rounds, u32* still, const SkCost C) {
	__shared__ long long wbest[SK_PICK_T / 64];
	const u32 lin = which[blockIdx.x], tid = threadIdx.x;
	if (!active[lin]) return;                              // (the whole workgroup)
	const NjFit q = fits[lin];
	const u32 m = q.m, nc = 2u * (m - 3u);
	ull* dl = delta + cand_off[lin];
	long long best = SK_KEY_NONE;                          // the order of (delta, v, k)
	for (u32 i = tid; i < nc; i += SK_PICK_T) {
		const long long key = (long long) dl[i] * SK_KEY_CAND + (long long) i;
		best = key < best ? key : best;
		dl[i] = 0;
	}
#pragma unroll
	for (int off = 32; off >= 1; off >>= 1) {
		const long long t = (long long) vdjx_shfl_xor64((u64) best, off);
		best = t < best ? t : best;
	}
	if ((tid & 63u) == 0) wbest[tid >> 6] = best;
	__syncthreads();
	best = wbest[0];
	for (u32 w = 1; w < SK_PICK_T / 64; w++) best = wbest[w] < best ? wbest[w] : best;
	const u32 cand = (u32) (best & (SK_KEY_CAND - 1));
	const long long d = (best - (long long) cand) / SK_KEY_CAND;
	if (tid == 0) rounds[lin]++;
	if (d >= 0) {
		if (tid == 0) active[lin] = 0;
		return;
	}
	u32* K = kid + 2u * q.node0;
	u32* U = par + q.node0;
	const u32 k = cand & 1u, v = sk_cand_node(m, q.root_kid, cand >> 1), p = U[v - m];
	const u32 s = K[2u * (p - m)] == v ? K[2u * (p - m) + 1u] : K[2u * (p - m)], c = K[2u * (v - m) + k], o = K[2u * (v - m) + 1u - k];
	__syncthreads();
	if (tid == 0) {
		K[2u * (v - m)] = min(s, o); K[2u * (v - m) + 1u] = max(s, o);
		K[2u * (p - m)] = min(c, v); K[2u * (p - m) + 1u] = max(c, v);
		if (s < m) leaf_par[q.first + s] = v; else U[s - m] = v;
		if (c < m) leaf_par[q.first + c] = p; else U[c - m] = p;
		W[lin] = (ull) ((long long) W[lin] + d);
		moves[lin]++;
		atomicAdd(still, 1u);
	}
	for (u32 col = tid; col < q.w; col += SK_PICK_T) {
		uint4* H = msg_all + q.fs_off + col;
		auto msg_of = [&](u32 y) { return y < m ? sk_leaf_msg(C, sk_code(contigs[ri[q.first + y].at + col])) : H[(size_t) (y - m) * q.w]; };
		const uint4 nv = sk_msg(C, sk_add(msg_of(s), msg_of(o)));
		uint4 nw = sk_msg(C, sk_add(msg_of(c), nv)), old = H[(size_t) (p - m) * q.w];
		H[(size_t) (v - m) * q.w] = nv;
		u32 x = p;
		while (sk_ne(nw, old)) {
			H[(size_t) (x - m) * q.w] = nw;
			const u32 g = U[x - m];
			if (g == q.root) break;
			nw = sk_msg(C, sk_add(nw, msg_of(K[2u * (g - m)] == x ? K[2u * (g - m) + 1u] : K[2u * (g - m)])));
			old = H[(size_t) (g - m) * q.w];
			x = g;
		}
	}
}

extern "C" int vdjx_sankoff_costs(const uint32_t* weight, uint32_t* cost, vdjx_sankoff_costs_info* info) {
	if (info) memset(info, 0, sizeof *info);
	if (!weight || !cost) { vdjx_set_error("vdjx_sankoff_costs: NULL argument"); return VDJX_EINVAL; }
	double mean;
	u32 lo, hi;
	sk_collapse(weight, cost, &mean, &lo, &hi);
	if (info) { info->mean = mean; info->min_cost = lo; info->max_cost = hi; }
	return VDJX_OK;
}

extern "C" int vdjx_tree_sankoff(vdjx_ctx* c, const char* contigs, size_t n, int len, const int32_t* clone, const int32_t* anchor, const uint32_t* prio,
                                 const uint32_t* cost, const int32_t* start_parent, const vdjx_tree_sankoff_params* params, int32_t* out_parent,
                                 int64_t* out_cost, int32_t* out_mutations, int32_t* out_depth, int32_t* out_clone, char* out_anc,
                                 vdjx_tree_sankoff_info* info) {
	static const char* who = "vdjx_tree_sankoff";
	if (info) memset(info, 0, sizeof *info);
	if (!c) { vdjx_set_error("%s: NULL argument", who); return VDJX_EINVAL; }
	if (params && (params->reserved[0] || params->reserved[1])) {
		vdjx_set_error("%s: params.reserved is {%u, %u} (it must be 0)", who, params->reserved[0], params->reserved[1]);
		return VDJX_EINVAL;
	}
	if (params && params->search > 1u) { vdjx_set_error("%s: params.search is %u (0: score the start tree, 1: search)", who, params->search); return VDJX_EINVAL; }
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
	const bool search = params ? params->search == 1u : true;
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
		if (q.m > NJ_MAX_M) {
			vdjx_set_error("%s: clone %d has %u members (at most %u)", who, clone[L.row_item[q.first]], q.m, NJ_MAX_M);
			return VDJX_ELIMIT;
		}
		inf0[k] = inf.internal;
		if (q.m >= 2) { big.push_back((u32) k); size.push_back(q.m); inf.edges += 2ull * q.m - 3; }
		if (q.m >= 3) inf.internal += q.m - 2;
		if (q.m >= 4 && search) inf.searched++;
	}
	const u64 nodes = (u64) n + inf.internal;
	// the start: vdjx_tree_mp's, checked as that call checks it, before this call's own GPU work
	std::vector<int32_t> nj_parent;
	if (!start_parent && !big.empty()) {
		nj_parent.resize((size_t) nodes);
		if (int rc = vdjx_nj_parents(c, contigs, n, len, clone, anchor, prio, nj_parent.data())) return rc;
	}
	const int32_t* start = start_parent ? start_parent : nj_parent.data();
	std::vector<int32_t> item_row(n, -1), lp;              // lp: the local parents of every lineage's nodes, lineage after lineage
	std::vector<u64> lp_off(L.clones.size());
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
	u64 steps_total = 0, w_final = 0;
	if (!big.empty()) {
		HIP_TRY(hipSetDevice(c->device));
		hipStream_t st = c->stream;
		vdjx_work wk(c);
		char *d_contigs, *d_anc = nullptr;
		TreeRow* d_ri;
		u32 *d_mut_row, *d_mut_inf, *d_leaf_par, *d_still;
		ull *d_cost_row, *d_cost_inf, *d_steps;
		HIP_TRY(wk.alloc(&d_contigs, n * (size_t) len));
		HIP_TRY(wk.alloc(&d_ri, (size_t) rows + 1));
		HIP_TRY(wk.alloc(&d_mut_row, rows));
		HIP_TRY(wk.alloc(&d_mut_inf, inf.internal));
		HIP_TRY(wk.alloc(&d_cost_row, rows));
		HIP_TRY(wk.alloc(&d_cost_inf, inf.internal));
		HIP_TRY(wk.alloc(&d_leaf_par, rows));
		HIP_TRY(wk.alloc(&d_still, 1));
		HIP_TRY(wk.alloc(&d_steps, SK_STEP_SLOTS));
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
		HIP_TRY(hipMemsetAsync(d_steps, 0, SK_STEP_SLOTS * sizeof(ull), st));
		const vdjx_arena::mark_t mk = wk.mark();
		std::vector<u32> h_kid, h_par, h_order, leaf_par(rows, 0u), cand_lin, cand_off, which, ones, h_moves, h_rounds;
		std::vector<ull> h_W, h_W0;
		std::vector<NjFit> fits;
		std::vector<NjFitItem> fit_items;
		volatile u32* h_still = (volatile u32*) (u32*) c->h_pin;
		for (size_t b = 0, k0 = 0; b < end.size(); k0 = end[b++]) {
			const size_t k1 = end[b], nl = k1 - k0;
			fits.clear(); fit_items.clear(); h_kid.clear(); h_par.clear(); h_order.clear(); which.clear();
			cand_lin.clear(); cand_off.assign(1, 0u);
			u64 fs_cells = 0;
			u32 max_tiles = 0;
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
				fits.push_back({fs_cells, q.first, m, q.w, (u32) (inf0[big[k]] - batch_inf0), root, t.root_kid, (u32) h_order.size(), 0u});
				h_order.insert(h_order.end(), t.order.begin(), t.order.end());
				const u32 tiles = (q.w + 63u) / 64u, nc = search && m > 3 ? 2u * (m - 3u) : 0u;
				for (u32 c0 = 0; c0 < q.w; c0 += 64u) fit_items.push_back({(u32) (k - k0), c0});
				cand_lin.insert(cand_lin.end(), nc, (u32) (k - k0));
				cand_off.push_back(cand_off.back() + nc);
				if (nc) { which.push_back((u32) (k - k0)); max_tiles = std::max(max_tiles, tiles); }
				fs_cells += (u64) (m - 2u) * q.w;
			}
			const u32 n_cand = cand_off.back();                  // (below 2^21: a call has fewer than 2^20 items)
			// the scorer's grid: a wave per candidate that walks all its column tiles, or as many waves per candidate as give SK_FILL_WAVES
			const u32 grid_y = n_cand ? std::min(max_tiles, (SK_FILL_WAVES + n_cand - 1u) / n_cand) : 1u;
			ones.assign(nl, 0u);
			for (u32 l : which) ones[l] = 1u;
			NjFit* d_fits;
			NjFitItem* d_fit_items;
			u32 *d_kid, *d_par, *d_order, *d_cand_lin, *d_cand_off, *d_which, *d_active, *d_moves, *d_rounds;
			ull *d_W, *d_delta;
			uint4* d_msg;
			uint8_t* d_state;
			HIP_TRY(wk.alloc(&d_fits, nl));
			HIP_TRY(wk.alloc(&d_fit_items, fit_items.size()));
			HIP_TRY(wk.alloc(&d_kid, h_kid.size()));
			HIP_TRY(wk.alloc(&d_par, h_par.size()));
			HIP_TRY(wk.alloc(&d_order, h_order.size()));
			HIP_TRY(wk.alloc(&d_cand_lin, n_cand));
			HIP_TRY(wk.alloc(&d_cand_off, nl + 1));
			HIP_TRY(wk.alloc(&d_which, which.size()));
			HIP_TRY(wk.alloc(&d_W, nl));
			HIP_TRY(wk.alloc(&d_active, nl));
			HIP_TRY(wk.alloc(&d_moves, nl));
			HIP_TRY(wk.alloc(&d_rounds, nl));
			HIP_TRY(wk.alloc(&d_delta, n_cand));
			HIP_TRY(wk.alloc(&d_msg, (size_t) fs_cells));
			HIP_TRY(wk.alloc(&d_state, (size_t) fs_cells));
			HIP_TRY(hipMemcpyAsync(d_fits, fits.data(), nl * sizeof(NjFit), hipMemcpyHostToDevice, st));
			HIP_TRY(hipMemcpyAsync(d_fit_items, fit_items.data(), fit_items.size() * sizeof(NjFitItem), hipMemcpyHostToDevice, st));
			if (!h_kid.empty()) {
				HIP_TRY(hipMemcpyAsync(d_kid, h_kid.data(), h_kid.size() * sizeof(u32), hipMemcpyHostToDevice, st));
				HIP_TRY(hipMemcpyAsync(d_par, h_par.data(), h_par.size() * sizeof(u32), hipMemcpyHostToDevice, st));
				HIP_TRY(hipMemcpyAsync(d_order, h_order.data(), h_order.size() * sizeof(u32), hipMemcpyHostToDevice, st));
			}
			HIP_TRY(hipMemcpyAsync(d_leaf_par + row0, leaf_par.data() + row0, (size_t) (row1 - row0) * sizeof(u32), hipMemcpyHostToDevice, st));
			if (n_cand) HIP_TRY(hipMemcpyAsync(d_cand_lin, cand_lin.data(), (size_t) n_cand * sizeof(u32), hipMemcpyHostToDevice, st));
			HIP_TRY(hipMemcpyAsync(d_cand_off, cand_off.data(), (nl + 1) * sizeof(u32), hipMemcpyHostToDevice, st));
			if (!which.empty()) HIP_TRY(hipMemcpyAsync(d_which, which.data(), which.size() * sizeof(u32), hipMemcpyHostToDevice, st));
			HIP_TRY(hipMemcpyAsync(d_active, ones.data(), nl * sizeof(u32), hipMemcpyHostToDevice, st));
			HIP_TRY(hipMemsetAsync(d_W, 0, nl * sizeof(ull), st));
			HIP_TRY(hipMemsetAsync(d_moves, 0, nl * sizeof(u32), st));
			HIP_TRY(hipMemsetAsync(d_rounds, 0, nl * sizeof(u32), st));
			HIP_TRY(hipMemsetAsync(d_delta, 0, (size_t) (n_cand ? n_cand : 1) * sizeof(ull), st));
			{
				vdjx_prof_scope ps(c, "k_sk_up");
				hipLaunchKernelGGL(k_sk_up, dim3((u32) fit_items.size()), dim3(64), 0, st, (const NjFitItem*) d_fit_items, (const NjFit*) d_fits, (const char*) d_contigs,
				                   (const TreeRow*) d_ri, (const u32*) d_kid, (const u32*) d_order, d_msg, d_W, C);
			}
			h_W0.resize(nl); h_W.resize(nl); h_moves.resize(nl); h_rounds.resize(nl);
			HIP_TRY(hipMemcpyAsync(h_W0.data(), d_W, nl * sizeof(ull), hipMemcpyDeviceToHost, st));
			HIP_TRY(hipStreamSynchronize(st));                  // (the host vectors above are free again; so is h_pin's first word)
			for (u32 round = 1; n_cand; round++) {
				HIP_TRY(hipMemsetAsync(d_still, 0, sizeof(u32), st));
				{
					vdjx_prof_scope ps(c, "k_sk_score");
					hipLaunchKernelGGL(k_sk_score, dim3(n_cand, grid_y), dim3(64), 0, st, (const NjFit*) d_fits, (const u32*) d_cand_lin, (const u32*) d_cand_off,
					                   (const char*) d_contigs, (const TreeRow*) d_ri, (const u32*) d_kid, (const u32*) d_par, (const uint4*) d_msg,
					                   (const u32*) d_active, d_delta, d_steps, C);
				}
				{
					vdjx_prof_scope ps(c, "k_sk_pick");
					hipLaunchKernelGGL(k_sk_pick, dim3((u32) which.size()), dim3(SK_PICK_T), 0, st, (const u32*) d_which, (const NjFit*) d_fits, (const u32*) d_cand_off,
					                   (const char*) d_contigs, (const TreeRow*) d_ri, d_kid, d_par, d_leaf_par, d_msg, d_W, d_active, d_delta, d_moves, d_rounds,
					                   d_still, C);
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
			if (!h_par.empty()) HIP_TRY(hipMemcpyAsync(h_par.data(), d_par, h_par.size() * sizeof(u32), hipMemcpyDeviceToHost, st));
			HIP_TRY(hipMemcpyAsync(leaf_par.data() + row0, d_leaf_par + row0, (size_t) (row1 - row0) * sizeof(u32), hipMemcpyDeviceToHost, st));
			HIP_TRY(hipStreamSynchronize(st));
			h_order.clear();
			std::vector<int32_t> fp;
			for (size_t k = k0; k < k1; k++) {
				const TreeClone& q = L.clones[big[k]];
				const NjFit& f = fits[k - k0];
				const u32 m = q.m, root = f.root;
				fp.assign(m < 3 ? m : 2 * m - 2, -1);
				for (u32 v = 0; v < (u32) fp.size(); v++)
					if (v != root) fp[v] = (int32_t) (v < m ? leaf_par[q.first + v] : h_par[f.node0 + v - m]);
				if (const int e = mp_orient(m, root, fp.data(), t)) {
					vdjx_set_error("%s: the searched parents of clone %d (%u members) are no tree: %s", who, clone[L.row_item[q.first]], m, mp_why(e));
					return VDJX_ESTATE;
				}
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
				if (search && m > 3) inf.candidates += (u64) h_rounds[k - k0] * 2u * (m - 3u);
			}
			if (!h_order.empty()) HIP_TRY(hipMemcpyAsync(d_order, h_order.data(), h_order.size() * sizeof(u32), hipMemcpyHostToDevice, st));
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
		std::vector<ull> cost_row(rows), cost_inf((size_t) inf.internal), h_steps(SK_STEP_SLOTS);
		HIP_TRY(hipMemcpyAsync(mut_row.data(), d_mut_row, (size_t) rows * sizeof(u32), hipMemcpyDeviceToHost, st));
		HIP_TRY(hipMemcpyAsync(cost_row.data(), d_cost_row, (size_t) rows * sizeof(ull), hipMemcpyDeviceToHost, st));
		if (inf.internal) {
			HIP_TRY(hipMemcpyAsync(mut_inf.data(), d_mut_inf, (size_t) inf.internal * sizeof(u32), hipMemcpyDeviceToHost, st));
			HIP_TRY(hipMemcpyAsync(cost_inf.data(), d_cost_inf, (size_t) inf.internal * sizeof(ull), hipMemcpyDeviceToHost, st));
		}
		HIP_TRY(hipMemcpyAsync(h_steps.data(), d_steps, SK_STEP_SLOTS * sizeof(ull), hipMemcpyDeviceToHost, st));
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
		for (ull s : h_steps) steps_total += s;
		if (inf.cost != w_final) {
			vdjx_set_error("%s: the search ended at a cost of %llu, the final trees' edges cost %llu", who, (ull) w_final, (ull) inf.cost);
			return VDJX_ESTATE;
		}
	}
	if (info) *info = inf;
	c->stats["tree_sankoff_candidates"] = inf.candidates;
	c->stats["tree_sankoff_steps"] = steps_total;
	c->stats["tree_sankoff_us"] = (u64) std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
	return VDJX_OK;
}
