// vdjx_mp.hip -- maximum-parsimony lineage trees by a search over nearest-neighbour interchanges (gfx950 only, wave64).
//
//   vdjx_tree_mp   per lineage: from vdjx_tree_nj's tree or the caller's, rounds that score every nearest-neighbour interchange by Fitch's
//                  union events over all window columns and apply the one of smallest key (P, v, k) while it lowers P; then Fitch's two
//                  passes on the final topology (the model: include/vdjx.h; in Python: tests/tree_mp_model.py)
//
// The host lays the members out as rows (vdjx_treelay.h), checks the start trees (vdjx_mp_host.h) and cuts the lineages of two and more
// into vdjx_tree_nj's batches.  A batch keeps on the device, per lineage, kid[2] and par of every inferred node, the parent of every leaf,
// one set per (inferred node, column) -- a byte, the column the fastest index --, its P and one int32 per candidate:
//   k_mp_up        one wave per (lineage, 64 columns), a lane per column: the sets in the host's post-order of the start tree, and P by
//                  one integer atomicAdd per wave of the ballots' popcounts
//   k_mp_score     the hot kernel.  One wave per (lineage, candidate) and column tile, or over several tiles in turn.  A swap at (v, k) changes only the sets of v, p and p's
//                  ancestors: every lane recomputes v' and p' and walks towards the root, combining the new set of the child on the path
//                  with the STORED set of the other child, and adds up (new union flag - old union flag); the root step ends the walk,
//                  and so does a ballot that says no lane's set differs from the stored one any more.  kid and par are read at
//                  wave-uniform addresses.  The wave's sum goes into the candidate's int32 by an integer atomicAdd (a sum: any order)
//   k_mp_pick      one workgroup per lineage that is still searching: the smallest (delta, candidate) by shuffles and four LDS slots; if
//                  the delta is negative one thread rewires kid and par, all threads rewrite the stored sets along the same path for
//                  every column, P follows, the lineage counts as still active; the deltas are cleared either way
// The host reads one counter per round (page-locked) and stops at 0 or at max_rounds; it reads kid and par back, roots them (O(nodes)) and
// runs k_nj_fitch (vdjx_fitch.h) on them.  No floating point, no spin-wait; nothing waits for another workgroup.  Scratch comes from the
// context's workspace.
#include "vdjx_common.h"
#include "vdjx_fitch.h"
#include "vdjx_link.h"
#include "vdjx_mp_host.h"
#include "vdjx_treelay.h"

#include <string.h>

static_assert(VDJX_MP_MAX_MEMBERS == NJ_MAX_M, "the header's limit");
#define MP_STEP_SLOTS 64u                // the step counter is spread over this many words
#define MP_FILL_WAVES 16384u             // 256 CUs x 4 SIMDs x 16 waves

// k_mp_up, mp_comb and mp_flag: vdjx_fitch.h (vdjx_spr.hip starts from the same sets)
// the j-th candidate node of a lineage: the inferred nodes but the root's child, ascending
__device__ inline u32 mp_cand_node(u32 m, u32 root_kid, u32 j) { return m + j + (m + j >= root_kid ? 1u : 0u); }

// blockIdx.x: a candidate of the batch, cand_lin[] its lineage, cand_off[nl + 1] the candidates of the lineages before.  The wave takes the
// column tiles blockIdx.y, blockIdx.y + gridDim.y, ...: the host makes the grid as high as it takes to fill the device and no higher (with
// a wave per tile a round of many small lineages was bound by the rate at which waves start)
__global__ __launch_bounds__(64) void k_mp_score(const NjFit* __restrict__ fits, const u32* __restrict__ cand_lin, const u32* __restrict__ cand_off,
                                                 const char* __restrict__ contigs, const TreeRow* __restrict__ ri, const u32* __restrict__ kid,
                                                 const u32* __restrict__ par, const uint8_t* __restrict__ up_all, const u32* __restrict__ active,
                                                 int* __restrict__ delta, unsigned long long* __restrict__ steps) {
	const u32 lin = cand_lin[blockIdx.x], lane = threadIdx.x;
	if (!active[lin]) return;
	const NjFit q = fits[lin];
	const u32 m = q.m, cand = blockIdx.x - cand_off[lin];
	if (blockIdx.y * 64u >= q.w) return;
	const u32* K = kid + 2u * q.node0;                     // K[2 (v - m)], K[2 (v - m) + 1]
	const u32* U = par + q.node0;
	const u32 k = cand & 1u, v = mp_cand_node(m, q.root_kid, cand >> 1), p = U[v - m];
	const u32 s = K[2u * (p - m)] == v ? K[2u * (p - m) + 1u] : K[2u * (p - m)], c = K[2u * (v - m) + k], o = K[2u * (v - m) + 1u - k];
	int d = 0;
	u32 made = 0;
	for (u32 col0 = blockIdx.y * 64u; col0 < q.w; col0 += gridDim.y * 64u) {
		const bool live = col0 + lane < q.w;
		const u32 cc = live ? col0 + lane : 0u;
		const uint8_t* up = up_all + q.fs_off + cc;
		auto leaf = [&](u32 y) { return nj_leaf_set(contigs[ri[q.first + y].at + cc]); };
		auto set_of = [&](u32 y) { return y < m ? leaf(y) : (u32) up[(size_t) (y - m) * q.w]; };
		const u32 Ss = set_of(s), Sc = set_of(c), So = set_of(o), Sv = set_of(v);
		const u32 nv = mp_comb(Ss, So);
		int dt = mp_flag(Ss, So) - mp_flag(Sc, So) + mp_flag(Sc, nv) - mp_flag(Sv, Ss);
		u32 x = p, old = set_of(p), nw = mp_comb(Sc, nv);
		made += 2u;
		while (__ballot(live && nw != old)) {
			const u32 g = U[x - m];
			if (g == q.root) {
				const u32 rs = leaf(g);
				dt += mp_flag(rs, nw) - mp_flag(rs, old);
				break;
			}
			const u32 a = set_of(K[2u * (g - m)] == x ? K[2u * (g - m) + 1u] : K[2u * (g - m)]);
			dt += mp_flag(nw, a) - mp_flag(old, a);
			nw = mp_comb(nw, a);
			old = set_of(g);
			x = g;
			made++;
		}
		d += live ? dt : 0;
	}
	d = vdjx_wave_sum(d);
	if (lane == 0) {
		if (d) atomicAdd(delta + blockIdx.x, d);
		atomicAdd(steps + ((blockIdx.x + blockIdx.y) % MP_STEP_SLOTS), (unsigned long long) made);
	}
}

#define MP_PICK_T 256
#define MP_KEY_NONE 0x7FFFFFFFFFFFFFFFll

// one workgroup per searched lineage (which[]).  kid, par and leaf_par are rewritten by thread 0 AFTER every thread has read the candidate's
// neighbourhood; what the threads read on their way up afterwards (par of p and above, kid above p) is nothing the move touches
__global__ __launch_bounds__(MP_PICK_T) void k_mp_pick(const u32* __restrict__ which, const NjFit* __restrict__ fits, const u32* __restrict__ cand_off,
                                                       const char* __restrict__ contigs, const TreeRow* __restrict__ ri, u32* kid, u32* par, u32* leaf_par,
                                                       uint8_t* up_all, u32* P, u32* active, int* delta, u32* moves, u32* rounds, u32* still) {
	__shared__ long long wbest[MP_PICK_T / 64];
	const u32 lin = which[blockIdx.x], tid = threadIdx.x;
	if (!active[lin]) return;                              // (the whole workgroup)
	const NjFit q = fits[lin];
	const u32 m = q.m, nc = 2u * (m - 3u);
	int* dl = delta + cand_off[lin];
	long long best = MP_KEY_NONE;                          // delta << 32 | candidate: the order of (delta, v, k)
	for (u32 i = tid; i < nc; i += MP_PICK_T) {
		const long long key = (long long) dl[i] * 4294967296ll + (long long) i;
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
	for (u32 w = 1; w < MP_PICK_T / 64; w++) best = wbest[w] < best ? wbest[w] : best;
	const u32 cand = (u32) (best & 0xFFFFFFFFll);
	const int d = (int) ((best - (long long) cand) / 4294967296ll);
	if (tid == 0) rounds[lin]++;
	if (d >= 0) {
		if (tid == 0) active[lin] = 0;
		return;
	}
	u32* K = kid + 2u * q.node0;
	u32* U = par + q.node0;
	const u32 k = cand & 1u, v = mp_cand_node(m, q.root_kid, cand >> 1), p = U[v - m];
	const u32 s = K[2u * (p - m)] == v ? K[2u * (p - m) + 1u] : K[2u * (p - m)], c = K[2u * (v - m) + k], o = K[2u * (v - m) + 1u - k];
	__syncthreads();
	if (tid == 0) {
		K[2u * (v - m)] = min(s, o); K[2u * (v - m) + 1u] = max(s, o);
		K[2u * (p - m)] = min(c, v); K[2u * (p - m) + 1u] = max(c, v);
		if (s < m) leaf_par[q.first + s] = v; else U[s - m] = v;
		if (c < m) leaf_par[q.first + c] = p; else U[c - m] = p;
		P[lin] = (u32) ((int) P[lin] + d);
		moves[lin]++;
		atomicAdd(still, 1u);
	}
	for (u32 col = tid; col < q.w; col += MP_PICK_T) {
		uint8_t* up = up_all + q.fs_off + col;
		auto set_of = [&](u32 y) { return y < m ? nj_leaf_set(contigs[ri[q.first + y].at + col]) : (u32) up[(size_t) (y - m) * q.w]; };
		const u32 Sc = set_of(c), nv = mp_comb(set_of(s), set_of(o));
		up[(size_t) (v - m) * q.w] = (uint8_t) nv;
		u32 x = p, old = set_of(p), nw = mp_comb(Sc, nv);
		while (nw != old) {
			up[(size_t) (x - m) * q.w] = (uint8_t) nw;
			const u32 g = U[x - m];
			if (g == q.root) break;
			nw = mp_comb(nw, set_of(K[2u * (g - m)] == x ? K[2u * (g - m) + 1u] : K[2u * (g - m)]));
			old = set_of(g);
			x = g;
		}
	}
}

extern "C" int vdjx_tree_mp(vdjx_ctx* c, const char* contigs, size_t n, int len, const int32_t* clone, const int32_t* anchor, const uint32_t* prio,
                            const int32_t* start_parent, const vdjx_tree_mp_params* params, int32_t* out_parent, int32_t* out_mutations,
                            int32_t* out_depth, int32_t* out_clone, char* out_anc, vdjx_tree_mp_info* info) {
	static const char* who = "vdjx_tree_mp";
	if (info) memset(info, 0, sizeof *info);
	if (!c) { vdjx_set_error("%s: NULL argument", who); return VDJX_EINVAL; }
	if (params && params->reserved) { vdjx_set_error("%s: params.reserved is %u (it must be 0)", who, params->reserved); return VDJX_EINVAL; }
	if (n == 0) return VDJX_OK;
	if (!contigs || !clone || !anchor || !out_parent || !out_mutations || !out_depth || !out_clone) {
		vdjx_set_error("%s: NULL argument", who);
		return VDJX_EINVAL;
	}
	if (int rc = tree_check_contigs(who, contigs, n, len)) return rc;
	const auto t0 = std::chrono::steady_clock::now();       // (where vdjx_tree_nj starts its clock)
	const u32 max_rounds = params ? params->max_rounds : 0u;
	std::vector<u64> keys;
	if (int rc = tree_keys(who, n, len, clone, anchor, keys)) return rc;
	const u32 rows = (u32) keys.size();
	TreeLay L;
	if (rows)
		if (int rc = tree_lay(who, keys, len, clone, anchor, prio, L)) return rc;
	vdjx_tree_mp_info inf;
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
		if (q.m >= 4) inf.searched++;
	}
	const u64 nodes = (u64) n + inf.internal;
	// the start: the caller's parents, or vdjx_tree_nj's for the same arguments (vdjx_nj_parents: the public function's own steps as far as
	// the parents, so its bits are the start; it leaves no statistic).  Either way every lineage's parents are checked before this call's
	// own GPU work
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
	for (u64 s = 0; s < nodes; s++) out_parent[s] = out_mutations[s] = out_depth[s] = out_clone[s] = -1;
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
	u64 steps_total = 0, p_final = 0;
	if (!big.empty()) {
		HIP_TRY(hipSetDevice(c->device));
		hipStream_t st = c->stream;
		vdjx_work wk(c);
		char *d_contigs, *d_anc = nullptr;
		TreeRow* d_ri;
		u32 *d_mut_row, *d_mut_inf, *d_leaf_par, *d_still;
		unsigned long long* d_steps;
		HIP_TRY(wk.alloc(&d_contigs, n * (size_t) len));
		HIP_TRY(wk.alloc(&d_ri, (size_t) rows + 1));
		HIP_TRY(wk.alloc(&d_mut_row, rows));
		HIP_TRY(wk.alloc(&d_mut_inf, inf.internal));
		HIP_TRY(wk.alloc(&d_leaf_par, rows));
		HIP_TRY(wk.alloc(&d_still, 1));
		HIP_TRY(wk.alloc(&d_steps, MP_STEP_SLOTS));
		if (out_anc && inf.internal) {
			HIP_TRY(wk.alloc(&d_anc, (size_t) inf.internal * (size_t) len));
			HIP_TRY(hipMemsetAsync(d_anc, 0, (size_t) inf.internal * (size_t) len, st));
		}
		HIP_TRY(hipMemcpyAsync(d_contigs, contigs, n * (size_t) len, hipMemcpyHostToDevice, st));
		HIP_TRY(hipMemcpyAsync(d_ri, L.ri.data(), ((size_t) rows + 1) * sizeof(TreeRow), hipMemcpyHostToDevice, st));
		HIP_TRY(hipMemsetAsync(d_mut_row, 0, (size_t) rows * sizeof(u32), st));
		HIP_TRY(hipMemsetAsync(d_mut_inf, 0, (size_t) (inf.internal ? inf.internal : 1) * sizeof(u32), st));
		HIP_TRY(hipMemsetAsync(d_steps, 0, MP_STEP_SLOTS * sizeof(unsigned long long), st));
		const vdjx_arena::mark_t mk = wk.mark();
		std::vector<u32> h_kid, h_par, h_order, leaf_par(rows, 0u), cand_lin, cand_off, which, ones, h_P, h_P0, h_moves, h_rounds;
		std::vector<NjFit> fits;
		std::vector<NjFitItem> fit_items;
		volatile u32* h_still = (volatile u32*) (u32*) c->h_pin;
		for (size_t b = 0, k0 = 0; b < end.size(); k0 = end[b++]) {
			const size_t k1 = end[b], nl = k1 - k0;
			fits.clear(); fit_items.clear(); h_kid.clear(); h_par.clear(); h_order.clear(); which.clear();
			cand_lin.clear(); cand_off.assign(1, 0u);
			u64 fs_bytes = 0;
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
				fits.push_back({fs_bytes, q.first, m, q.w, (u32) (inf0[big[k]] - batch_inf0), root, t.root_kid, (u32) h_order.size(), 0u});
				h_order.insert(h_order.end(), t.order.begin(), t.order.end());
				const u32 tiles = (q.w + 63u) / 64u, nc = m > 3 ? 2u * (m - 3u) : 0u;
				for (u32 c0 = 0; c0 < q.w; c0 += 64u) fit_items.push_back({(u32) (k - k0), c0});
				cand_lin.insert(cand_lin.end(), nc, (u32) (k - k0));
				cand_off.push_back(cand_off.back() + nc);
				if (nc) { which.push_back((u32) (k - k0)); max_tiles = std::max(max_tiles, tiles); }
				fs_bytes += (u64) (m - 2u) * q.w;
			}
			const u32 n_cand = cand_off.back();                  // (below 2^21: a call has fewer than 2^20 items)
			// the scorer's grid: a wave per candidate that walks all its column tiles, or as many waves per candidate as give MP_FILL_WAVES
			const u32 grid_y = n_cand ? std::min(max_tiles, (MP_FILL_WAVES + n_cand - 1u) / n_cand) : 1u;
			ones.assign(nl, 0u);
			for (u32 l : which) ones[l] = 1u;
			NjFit* d_fits;
			NjFitItem* d_fit_items;
			u32 *d_kid, *d_par, *d_order, *d_cand_lin, *d_cand_off, *d_which, *d_P, *d_active, *d_moves, *d_rounds;
			int* d_delta;
			uint8_t* d_up;
			HIP_TRY(wk.alloc(&d_fits, nl));
			HIP_TRY(wk.alloc(&d_fit_items, fit_items.size()));
			HIP_TRY(wk.alloc(&d_kid, h_kid.size()));
			HIP_TRY(wk.alloc(&d_par, h_par.size()));
			HIP_TRY(wk.alloc(&d_order, h_order.size()));
			HIP_TRY(wk.alloc(&d_cand_lin, n_cand));
			HIP_TRY(wk.alloc(&d_cand_off, nl + 1));
			HIP_TRY(wk.alloc(&d_which, which.size()));
			HIP_TRY(wk.alloc(&d_P, nl));
			HIP_TRY(wk.alloc(&d_active, nl));
			HIP_TRY(wk.alloc(&d_moves, nl));
			HIP_TRY(wk.alloc(&d_rounds, nl));
			HIP_TRY(wk.alloc(&d_delta, n_cand));
			HIP_TRY(wk.alloc(&d_up, (size_t) fs_bytes));
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
			HIP_TRY(hipMemsetAsync(d_P, 0, nl * sizeof(u32), st));
			HIP_TRY(hipMemsetAsync(d_moves, 0, nl * sizeof(u32), st));
			HIP_TRY(hipMemsetAsync(d_rounds, 0, nl * sizeof(u32), st));
			HIP_TRY(hipMemsetAsync(d_delta, 0, (size_t) (n_cand ? n_cand : 1) * sizeof(int), st));
			{
				vdjx_prof_scope ps(c, "k_mp_up");
				hipLaunchKernelGGL(k_mp_up, dim3((u32) fit_items.size()), dim3(64), 0, st, (const NjFitItem*) d_fit_items, (const NjFit*) d_fits, (const char*) d_contigs,
				                   (const TreeRow*) d_ri, (const u32*) d_kid, (const u32*) d_order, d_up, d_P);
			}
			h_P0.resize(nl); h_P.resize(nl); h_moves.resize(nl); h_rounds.resize(nl);
			HIP_TRY(hipMemcpyAsync(h_P0.data(), d_P, nl * sizeof(u32), hipMemcpyDeviceToHost, st));
			HIP_TRY(hipStreamSynchronize(st));                  // (the host vectors above are free again; so is h_pin's first word)
			for (u32 round = 1; n_cand; round++) {
				HIP_TRY(hipMemsetAsync(d_still, 0, sizeof(u32), st));
				{
					vdjx_prof_scope ps(c, "k_mp_score");
					hipLaunchKernelGGL(k_mp_score, dim3(n_cand, grid_y), dim3(64), 0, st, (const NjFit*) d_fits, (const u32*) d_cand_lin, (const u32*) d_cand_off,
					                   (const char*) d_contigs, (const TreeRow*) d_ri, (const u32*) d_kid, (const u32*) d_par, (const uint8_t*) d_up,
					                   (const u32*) d_active, d_delta, d_steps);
				}
				{
					vdjx_prof_scope ps(c, "k_mp_pick");
					hipLaunchKernelGGL(k_mp_pick, dim3((u32) which.size()), dim3(MP_PICK_T), 0, st, (const u32*) d_which, (const NjFit*) d_fits, (const u32*) d_cand_off,
					                   (const char*) d_contigs, (const TreeRow*) d_ri, d_kid, d_par, d_leaf_par, d_up, d_P, d_active, d_delta, d_moves, d_rounds, d_still);
				}
				HIP_TRY(hipMemcpyAsync((void*) h_still, d_still, sizeof(u32), hipMemcpyDeviceToHost, st));
				HIP_TRY(hipStreamSynchronize(st));
				HIP_TRY(hipGetLastError());
				if (*h_still == 0 || round == max_rounds) break;
			}
			// the host's part: root every lineage's final parents, fill the outputs that need no sequence, give Fitch's passes their order
			HIP_TRY(hipMemcpyAsync(h_P.data(), d_P, nl * sizeof(u32), hipMemcpyDeviceToHost, st));
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
				inf.parsimony_start += h_P0[k - k0];
				p_final += h_P[k - k0];
				inf.moves += h_moves[k - k0];
				inf.moved += h_moves[k - k0] > 0;
				inf.rounds = std::max(inf.rounds, h_rounds[k - k0]);
				if (m > 3) inf.candidates += (u64) h_rounds[k - k0] * 2u * (m - 3u);
			}
			if (!h_order.empty()) HIP_TRY(hipMemcpyAsync(d_order, h_order.data(), h_order.size() * sizeof(u32), hipMemcpyHostToDevice, st));
			{
				vdjx_prof_scope ps(c, "k_nj_fitch");
				hipLaunchKernelGGL(k_nj_fitch, dim3((u32) fit_items.size()), dim3(64), 0, st, (const NjFitItem*) d_fit_items, (const NjFit*) d_fits, (const char*) d_contigs,
				                   (const TreeRow*) d_ri, (const u32*) d_kid, (const u32*) d_par, (const u32*) d_order, (const u32*) d_leaf_par, d_up, d_mut_row,
				                   d_mut_inf + batch_inf0, d_anc ? d_anc + (size_t) batch_inf0 * (size_t) len : nullptr, (u32) len);
			}
			HIP_TRY(hipStreamSynchronize(st));                  // (the host vectors are uploaded from again, and the workspace is given up)
			HIP_TRY(hipGetLastError());
			vdjx_prof_collect(c, false);
			wk.release_to(mk);
		}
		std::vector<u32> mut_row(rows), mut_inf((size_t) inf.internal);
		std::vector<unsigned long long> h_steps(MP_STEP_SLOTS);
		HIP_TRY(hipMemcpyAsync(mut_row.data(), d_mut_row, (size_t) rows * sizeof(u32), hipMemcpyDeviceToHost, st));
		if (inf.internal) HIP_TRY(hipMemcpyAsync(mut_inf.data(), d_mut_inf, (size_t) inf.internal * sizeof(u32), hipMemcpyDeviceToHost, st));
		HIP_TRY(hipMemcpyAsync(h_steps.data(), d_steps, MP_STEP_SLOTS * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
		if (d_anc) HIP_TRY(hipMemcpyAsync(out_anc, d_anc, (size_t) inf.internal * (size_t) len, hipMemcpyDeviceToHost, st));
		HIP_TRY(hipStreamSynchronize(st));
		for (u32 r = 0; r < rows; r++) {
			const u32 i = L.row_item[r];
			if (out_parent[i] < 0) continue;
			out_mutations[i] = (int32_t) mut_row[r];
			inf.parsimony += mut_row[r];
		}
		for (u64 a = 0; a < inf.internal; a++) {
			out_mutations[n + a] = (int32_t) mut_inf[a];
			inf.parsimony += mut_inf[a];
		}
		for (unsigned long long s : h_steps) steps_total += s;
		if (inf.parsimony != p_final) {
			vdjx_set_error("%s: the search ended at %llu union events, the final trees have %llu mutations", who, (unsigned long long) p_final,
			               (unsigned long long) inf.parsimony);
			return VDJX_ESTATE;
		}
	}
	if (info) *info = inf;
	c->stats["tree_mp_candidates"] = inf.candidates;
	c->stats["tree_mp_steps"] = steps_total;
	c->stats["tree_mp_us"] = (u64) std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
	return VDJX_OK;
}
