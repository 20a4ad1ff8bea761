// vdjx_spr.hip -- maximum-parsimony lineage trees by a search over subtree prunings and regraftings (gfx950 only, wave64).
//
//   vdjx_tree_spr  per lineage: from vdjx_tree_nj's tree or the caller's, rounds that score every candidate (c, y) -- prune the subtree of
//                  c, regraft it on the edge above y -- by Fitch's union events over all window columns and apply the one of smallest key
//                  (P, c, y) while it lowers P; then Fitch's two passes on the final topology (the model: include/vdjx.h; in Python:
//                  tests/tree_spr_model.py)
//
// Everything around the search is vdjx_tree_mp's (vdjx_mp.hip): the layout, the start's check, the batches, kid[2] and par of every inferred
// node, the parent of every leaf and one up set per (inferred node, column) on the device -- and here the root's child too, which a move
// can change.  A round of a batch:
//   k_spr_score    the hot kernel.  One wave per (lineage, pruned node c), a lane per column, the lineage's column tiles in turn.  Per tile
//                  the walk from g = parent(parent(c)) to the root gives the up sets U' of T' (the tree without c's subtree) on that path
//                  and the part of the score that is the same for every y; then a stackless pre-order walk of T' over kid / par (wave-
//                  uniform addresses, c's parent transparent, c's subtree never entered) gives every node's down set D' and adds the
//                  popcount of the ballot "comb(U'(y), D'(y)) and U(c) do not meet" into y's int32 in LDS.  A byte per (node, lane) holds
//                  first U' in its high half -- the tile's stored sets are copied in, the path walk writes over them --, then D' in its
//                  low half: never both.  The store of D'(y) clears the high half; that is sound because every read of U'(y) -- the last one
//                  when y's parent is expanded -- comes before D'(y) is written, and the slab is filled again for every tile.  So the walks read no
//                  global memory but kid / par.  The slab is in LDS up to VDJX_SPR_LDS_MEMBERS members, in
//                  the workspace beyond (a slab per launched workgroup, the grid capped, a workgroup strides over the prunes).  After the
//                  last tile the wave reduces (sum, y) to c's 64-bit key
//   k_spr_pick     one workgroup per lineage still searching: the smallest key (delta, c, y); if the delta is negative all threads
//                  rewrite the stored up sets on the path above the pruned place, one thread rewires kid, par, the leaves' parents and
//                  the root's child, all threads rewrite the sets from the regrafted place up; P, the moves and the still-searching
//                  counter follow
// The host reads one counter per round (page-locked) and stops at 0 or at max_rounds; it reads kid and par back, roots them (O(nodes)) and
// runs k_nj_fitch (vdjx_fitch.h) on them.  No floating point, no spin-wait; nothing waits for another workgroup.  Integer atomics are sums
// only.  Scratch comes from the context's workspace.
#include "vdjx_common.h"
#include "vdjx_fitch.h"
#include "vdjx_link.h"
#include "vdjx_mp_host.h"
#include "vdjx_spr_host.h"
#include "vdjx_treelay.h"

#include <string.h>

static_assert(VDJX_SPR_MAX_MEMBERS <= NJ_MAX_M, "a searched lineage is one vdjx_tree_nj takes");
static_assert(2u * VDJX_SPR_MAX_MEMBERS - 2u < 65536u, "c and y share the low word of a key, 16 bits each");
#define VDJX_SPR_LDS_MEMBERS 128u        // the largest lineage whose slab k_spr_score keeps in LDS
#define SPR_SLAB_WGS 256u                // beyond it: the workgroups launched, each with a slab in the workspace (one per CU)
#define SPR_PICK_T 256
#define SPR_SUM_NONE 0x3FFFFFFF          // an int32 no tile has added to: the node is no y of this prune
#define SPR_KEY_NONE 0x7FFFFFFFFFFFFFFFll
// per node of a lineage: 64 slab bytes (a byte per lane: two sets of 4 bits) and an int32 sum.  160 KiB of LDS and 8 waves per CU wanted
// (2 per SIMD) leave 20 KiB a wave
#define SPR_NODE_LDS_BYTES 68u
static_assert(2u * VDJX_SPR_LDS_MEMBERS * SPR_NODE_LDS_BYTES <= 20480u, "8 waves per CU keep their slabs in 160 KiB of LDS");
static_assert(2u * VDJX_SPR_MAX_MEMBERS * (SPR_NODE_LDS_BYTES - 64u) <= 65536u, "the sums of the largest lineage fit a workgroup's LDS");

// lst[0 .. n_lst): the batch's units (a unit: a lineage and a node c of it, unit_lin / unit_off as k_mp_score's cand_lin / cand_off) of
// this launch.  cap: the nodes the launch's LDS (and slab) is cut for, a multiple of 4.  IN_LDS: the slab follows the sums in
// LDS; otherwise it is slabs + blockIdx.x * cap * 64.  keys[unit]: written for every unit of an active lineage, SPR_KEY_NONE where c is
// no pruned node or has no y
template <bool IN_LDS>
__global__ __launch_bounds__(64) void k_spr_score(const u32* __restrict__ lst, u32 n_lst, const u32* __restrict__ unit_lin, const u32* __restrict__ unit_off,
                                                  const NjFit* __restrict__ fits, const char* __restrict__ contigs, const TreeRow* __restrict__ ri,
                                                  const u32* __restrict__ kid, const u32* __restrict__ par, const u32* __restrict__ leaf_par,
                                                  const u32* __restrict__ rootkid, const uint8_t* __restrict__ up_all, const u32* __restrict__ active,
                                                  long long* __restrict__ keys, unsigned long long* __restrict__ cands, uint8_t* __restrict__ slabs, u32 cap) {
	extern __shared__ int spr_lds[];
	int* sums = spr_lds;
	uint8_t* slab = IN_LDS ? (uint8_t*) (sums + cap) : slabs + (size_t) blockIdx.x * cap * 64u;
	const u32 lane = threadIdx.x;
	for (u32 i = blockIdx.x; i < n_lst; i += gridDim.x) {
		const u32 unit = lst[i], lin = unit_lin[unit];
		if (!active[lin]) continue;                          // (the whole wave)
		const NjFit q = fits[lin];
		const u32 m = q.m, nodes = 2u * m - 2u, c = unit - unit_off[lin], rk = rootkid[lin];
		if (c == q.root || c == rk) {
			if (lane == 0) keys[unit] = SPR_KEY_NONE;
			continue;
		}
		const u32* K = kid + 2u * q.node0;                   // K[2 (v - m)], K[2 (v - m) + 1]
		const u32* U = par + q.node0;
		const u32 p = c < m ? leaf_par[q.first + c] : U[c - m];                      // (an inferred node: c is not the root's child)
		const u32 s = K[2u * (p - m)] == c ? K[2u * (p - m) + 1u] : K[2u * (p - m)], g = U[p - m];
		const u32 top = rk == p ? s : rk;                    // the root's child in T'
		__syncthreads();                                     // (the unit before has read its sums)
		for (u32 v = lane; v < nodes; v += 64u) sums[v] = SPR_SUM_NONE;
		__syncthreads();
		int cst = 0;
		u32 ncand = 0;
		for (u32 col0 = 0; col0 < q.w; col0 += 64u) {
			const bool live = col0 + lane < q.w, first = col0 == 0;
			const u32 cc = live ? col0 + lane : 0u;
			const uint8_t* up = up_all + q.fs_off + cc;
			auto leaf = [&](u32 y) { return nj_leaf_set(contigs[ri[q.first + y].at + cc]); };
			// the tile's stored sets of every node into the high halves of the slab's bytes: loads that do not wait for one another.  The
			// walks below then read a lane's own bytes only
#pragma unroll 4
			for (u32 v = 0; v < m; v++) slab[(size_t) v * 64u + lane] = (uint8_t) (leaf(v) << 4);
#pragma unroll 4
			for (u32 v = m; v < nodes; v++) slab[(size_t) v * 64u + lane] = (uint8_t) ((u32) up[(size_t) (v - m) * q.w] << 4);
			// up_t(y) is valid until D'(y) is stored over the byte (below): every use comes before that store
			auto up_t = [&](u32 y) { return (u32) slab[(size_t) y * 64u + lane] >> 4; };
			const u32 Sc = up_t(c), Ss = up_t(s), rs = up_t(q.root);
			// T' against T: p's union event goes, the events on the path from g up and the root step change.  U' of the path over U
			int dt = -mp_flag(Sc, Ss);
			u32 prev = p, nw = Ss, old = up_t(p);
			for (u32 x = g; x != q.root; x = U[x - m]) {
				const u32 a = up_t(K[2u * (x - m)] == prev ? K[2u * (x - m) + 1u] : K[2u * (x - m)]);
				dt += mp_flag(nw, a) - mp_flag(old, a);
				nw = mp_comb(nw, a);
				old = up_t(x);
				slab[(size_t) x * 64u + lane] = (uint8_t) (nw << 4);
				prev = x;
			}
			dt += mp_flag(rs, nw) - mp_flag(rs, old);
			cst += live ? dt : 0;
			auto score = [&](u32 y, u32 Uy, u32 Dy) {            // (y, its sets: wave-uniform y)
				if (y == s) return;                              // the edge above s is the old place
				const int cnt = __popcll(__ballot(live && !(mp_comb(Uy, Dy) & Sc)));
				if (lane == 0) sums[y] = first ? cnt : sums[y] + cnt;
				ncand += first ? 1u : 0u;
			};
			score(top, up_t(top), rs);
			slab[(size_t) top * 64u + lane] = (uint8_t) rs;
			u32 x = top;
			while (x >= m) {                                     // expand x: its children's D', their scores
				u32 a = K[2u * (x - m)], b = K[2u * (x - m) + 1u];
				a = a == p ? s : a;
				b = b == p ? s : b;
				const u32 Dx = slab[(size_t) x * 64u + lane] & 15u, Ua = up_t(a), Ub = up_t(b);
				const u32 Da = mp_comb(Dx, Ub), Db = mp_comb(Dx, Ua);
				score(a, Ua, Da);
				score(b, Ub, Db);
				slab[(size_t) a * 64u + lane] = (uint8_t) Da;      // (U' of a and b, read above, is not needed again)
				slab[(size_t) b * 64u + lane] = (uint8_t) Db;
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
		const int total = vdjx_wave_sum(cst);
		long long best = SPR_KEY_NONE;                       // delta << 32 | c << 16 | y: the order of (delta, c, y)
		for (u32 v = lane; v < nodes; v += 64u) {
			const int sv = sums[v];
			if (sv == SPR_SUM_NONE) continue;
			const long long key = (long long) (total + sv) * 4294967296ll + (long long) (c << 16 | v);
			best = key < best ? key : best;
		}
#pragma unroll
		for (int off = 32; off >= 1; off >>= 1) {
			const long long t = (long long) vdjx_shfl_xor64((u64) best, off);
			best = t < best ? t : best;
		}
		if (lane == 0) {
			keys[unit] = best;
			if (ncand) atomicAdd(cands + lin, (unsigned long long) ncand);
		}
	}
}

// one workgroup per searched lineage (which[]).  The sets above the pruned place are rewritten on the old kid / par; thread 0 rewires
// between two barriers; the sets from the regrafted place up are rewritten on the new ones.  A walk ends where a node's set comes out as
// stored: nothing above it changes
__global__ __launch_bounds__(SPR_PICK_T) void k_spr_pick(const u32* __restrict__ which, const NjFit* __restrict__ fits, const u32* __restrict__ unit_off,
                                                         const char* __restrict__ contigs, const TreeRow* __restrict__ ri, u32* kid, u32* par, u32* leaf_par,
                                                         u32* rootkid, uint8_t* up_all, u32* P, u32* active, const long long* __restrict__ keys, u32* moves,
                                                         u32* rounds, u32* still) {
	__shared__ long long wbest[SPR_PICK_T / 64];
	const u32 lin = which[blockIdx.x], tid = threadIdx.x;
	if (!active[lin]) return;                              // (the whole workgroup)
	const NjFit q = fits[lin];
	const u32 m = q.m, nodes = 2u * m - 2u;
	const long long* kl = keys + unit_off[lin];
	long long best = SPR_KEY_NONE;
	for (u32 i = tid; i < nodes; i += SPR_PICK_T) best = kl[i] < best ? kl[i] : best;
#pragma unroll
	for (int off = 32; off >= 1; off >>= 1) {
		const long long t = (long long) vdjx_shfl_xor64((u64) best, off);
		best = t < best ? t : best;
	}
	if ((tid & 63u) == 0) wbest[tid >> 6] = best;
	__syncthreads();
	best = wbest[0];
	for (u32 w = 1; w < SPR_PICK_T / 64; w++) best = wbest[w] < best ? wbest[w] : best;
	const u32 low = (u32) (best & 0xFFFFFFFFll);
	const int d = best == SPR_KEY_NONE ? 0 : (int) ((best - (long long) low) / 4294967296ll);
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
	auto set_of = [&](u32 v, u32 col) { return v < m ? nj_leaf_set(contigs[ri[q.first + v].at + col]) : (u32) up_all[q.fs_off + (size_t) (v - m) * q.w + col]; };
	for (u32 col = tid; col < q.w; col += SPR_PICK_T) {   // s in p's place: the sets from g up
		uint8_t* up = up_all + q.fs_off + col;
		u32 prev = p, nw = set_of(s, col), old = set_of(p, col);
		for (u32 z = g; z != q.root && nw != old; z = U[z - m]) {
			nw = mp_comb(nw, set_of(K[2u * (z - m)] == prev ? K[2u * (z - m) + 1u] : K[2u * (z - m)], col));
			old = up[(size_t) (z - m) * q.w];
			up[(size_t) (z - m) * q.w] = (uint8_t) nw;
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
		P[lin] = (u32) ((int) P[lin] + d);
		moves[lin]++;
		atomicAdd(still, 1u);
	}
	__syncthreads();
	for (u32 col = tid; col < q.w; col += SPR_PICK_T) {   // p above y: the sets from p up
		uint8_t* up = up_all + q.fs_off + col;
		u32 prev = p, nw = mp_comb(set_of(c, col), set_of(y, col));
		up[(size_t) (p - m) * q.w] = (uint8_t) nw;
		for (u32 z = x; z != q.root; z = U[z - m]) {
			nw = mp_comb(nw, set_of(K[2u * (z - m)] == prev ? K[2u * (z - m) + 1u] : K[2u * (z - m)], col));
			if (nw == (u32) up[(size_t) (z - m) * q.w]) break;
			up[(size_t) (z - m) * q.w] = (uint8_t) nw;
			prev = z;
		}
	}
}

extern "C" int vdjx_tree_spr(vdjx_ctx* c, const char* contigs, size_t n, int len, const int32_t* clone, const int32_t* anchor, const uint32_t* prio,
                             const int32_t* start_parent, const vdjx_tree_spr_params* params, int32_t* out_parent, int32_t* out_mutations,
                             int32_t* out_depth, int32_t* out_clone, char* out_anc, vdjx_tree_spr_info* info) {
	static const char* who = "vdjx_tree_spr";
	if (info) memset(info, 0, sizeof *info);
	if (!c) { vdjx_set_error("%s: NULL argument", who); return VDJX_EINVAL; }
	if (params && params->reserved) { vdjx_set_error("%s: params.reserved is %u (it must be 0)", who, params->reserved); return VDJX_EINVAL; }
	if (n == 0) return VDJX_OK;
	if (!contigs || !clone || !anchor || !out_parent || !out_mutations || !out_depth || !out_clone) {
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
	vdjx_tree_spr_info inf;
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
	u64 p_final = 0;
	if (!big.empty()) {
		HIP_TRY(hipSetDevice(c->device));
		hipStream_t st = c->stream;
		vdjx_work wk(c);
		char *d_contigs, *d_anc = nullptr;
		TreeRow* d_ri;
		u32 *d_mut_row, *d_mut_inf, *d_leaf_par, *d_still;
		HIP_TRY(wk.alloc(&d_contigs, n * (size_t) len));
		HIP_TRY(wk.alloc(&d_ri, (size_t) rows + 1));
		HIP_TRY(wk.alloc(&d_mut_row, rows));
		HIP_TRY(wk.alloc(&d_mut_inf, inf.internal));
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
		const vdjx_arena::mark_t mk = wk.mark();
		std::vector<u32> h_kid, h_par, h_order, leaf_par(rows, 0u), unit_lin, unit_off, lst_lds, lst_slab, which, ones, h_rootkid, h_P, h_P0, h_moves, h_rounds;
		std::vector<unsigned long long> h_cands;
		std::vector<NjFit> fits;
		std::vector<NjFitItem> fit_items;
		volatile u32* h_still = (volatile u32*) (u32*) c->h_pin;
		for (size_t b = 0, k0 = 0; b < end.size(); k0 = end[b++]) {
			const size_t k1 = end[b], nl = k1 - k0;
			fits.clear(); fit_items.clear(); h_kid.clear(); h_par.clear(); h_order.clear(); which.clear(); h_rootkid.clear();
			unit_lin.clear(); unit_off.assign(1, 0u); lst_lds.clear(); lst_slab.clear();
			u64 fs_bytes = 0;
			u32 m_lds = 0, m_slab = 0;                           // the largest searched lineage on either side of the bound
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
				fits.push_back({fs_bytes, q.first, m, q.w, (u32) (inf0[big[k]] - batch_inf0), root, t.root_kid, (u32) h_order.size(), 0u});
				h_order.insert(h_order.end(), t.order.begin(), t.order.end());
				for (u32 c0 = 0; c0 < q.w; c0 += 64u) fit_items.push_back({(u32) (k - k0), c0});
				const u32 nu = m > 3 ? 2u * m - 2u : 0u;          // a unit per node: the root leaf's and its child's write an empty key
				for (u32 v = 0; v < nu; v++) (m <= VDJX_SPR_LDS_MEMBERS ? lst_lds : lst_slab).push_back(unit_off.back() + v);
				unit_lin.insert(unit_lin.end(), nu, (u32) (k - k0));
				unit_off.push_back(unit_off.back() + nu);
				if (nu) {
					which.push_back((u32) (k - k0));
					if (m <= VDJX_SPR_LDS_MEMBERS) m_lds = std::max(m_lds, m); else m_slab = std::max(m_slab, m);
				}
				fs_bytes += (u64) (m - 2u) * q.w;
			}
			const u32 n_unit = unit_off.back();                  // (below 2^21: a call has fewer than 2^20 items)
			const u32 cap_lds = (2u * m_lds + 1u) & ~3u, cap_slab = (2u * m_slab + 1u) & ~3u;      // 2m - 2 nodes, up to a multiple of 4
			const u32 grid_slab = std::min((u32) lst_slab.size(), SPR_SLAB_WGS);
			ones.assign(nl, 0u);
			for (u32 l : which) ones[l] = 1u;
			NjFit* d_fits;
			NjFitItem* d_fit_items;
			u32 *d_kid, *d_par, *d_order, *d_unit_lin, *d_unit_off, *d_lst_lds, *d_lst_slab, *d_which, *d_rootkid, *d_P, *d_active, *d_moves, *d_rounds;
			long long* d_keys;
			unsigned long long* d_cands;
			uint8_t *d_up, *d_slabs;
			HIP_TRY(wk.alloc(&d_fits, nl));
			HIP_TRY(wk.alloc(&d_fit_items, fit_items.size()));
			HIP_TRY(wk.alloc(&d_kid, h_kid.size()));
			HIP_TRY(wk.alloc(&d_par, h_par.size()));
			HIP_TRY(wk.alloc(&d_order, h_order.size()));
			HIP_TRY(wk.alloc(&d_unit_lin, n_unit));
			HIP_TRY(wk.alloc(&d_unit_off, nl + 1));
			HIP_TRY(wk.alloc(&d_lst_lds, lst_lds.size()));
			HIP_TRY(wk.alloc(&d_lst_slab, lst_slab.size()));
			HIP_TRY(wk.alloc(&d_which, which.size()));
			HIP_TRY(wk.alloc(&d_rootkid, nl));
			HIP_TRY(wk.alloc(&d_P, nl));
			HIP_TRY(wk.alloc(&d_active, nl));
			HIP_TRY(wk.alloc(&d_moves, nl));
			HIP_TRY(wk.alloc(&d_rounds, nl));
			HIP_TRY(wk.alloc(&d_keys, n_unit));
			HIP_TRY(wk.alloc(&d_cands, nl));
			HIP_TRY(wk.alloc(&d_up, (size_t) fs_bytes));
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
			if (!lst_lds.empty()) HIP_TRY(hipMemcpyAsync(d_lst_lds, lst_lds.data(), lst_lds.size() * sizeof(u32), hipMemcpyHostToDevice, st));
			if (!lst_slab.empty()) HIP_TRY(hipMemcpyAsync(d_lst_slab, lst_slab.data(), lst_slab.size() * sizeof(u32), hipMemcpyHostToDevice, st));
			if (!which.empty()) HIP_TRY(hipMemcpyAsync(d_which, which.data(), which.size() * sizeof(u32), hipMemcpyHostToDevice, st));
			HIP_TRY(hipMemcpyAsync(d_rootkid, h_rootkid.data(), nl * sizeof(u32), hipMemcpyHostToDevice, st));
			HIP_TRY(hipMemcpyAsync(d_active, ones.data(), nl * sizeof(u32), hipMemcpyHostToDevice, st));
			HIP_TRY(hipMemsetAsync(d_P, 0, nl * sizeof(u32), st));
			HIP_TRY(hipMemsetAsync(d_moves, 0, nl * sizeof(u32), st));
			HIP_TRY(hipMemsetAsync(d_rounds, 0, nl * sizeof(u32), st));
			HIP_TRY(hipMemsetAsync(d_cands, 0, nl * sizeof(unsigned long long), st));
			{
				vdjx_prof_scope ps(c, "k_mp_up");
				hipLaunchKernelGGL(k_mp_up, dim3((u32) fit_items.size()), dim3(64), 0, st, (const NjFitItem*) d_fit_items, (const NjFit*) d_fits, (const char*) d_contigs,
				                   (const TreeRow*) d_ri, (const u32*) d_kid, (const u32*) d_order, d_up, d_P);
			}
			h_P0.resize(nl); h_P.resize(nl); h_moves.resize(nl); h_rounds.resize(nl); h_cands.resize(nl);
			HIP_TRY(hipMemcpyAsync(h_P0.data(), d_P, nl * sizeof(u32), hipMemcpyDeviceToHost, st));
			HIP_TRY(hipStreamSynchronize(st));                  // (the host vectors above are free again; so is h_pin's first word)
			for (u32 round = 1; n_unit; round++) {
				HIP_TRY(hipMemsetAsync(d_still, 0, sizeof(u32), st));
				if (!lst_lds.empty()) {
					vdjx_prof_scope ps(c, "k_spr_score");
					hipLaunchKernelGGL(k_spr_score<true>, dim3((u32) lst_lds.size()), dim3(64), cap_lds * SPR_NODE_LDS_BYTES, st, (const u32*) d_lst_lds, (u32) lst_lds.size(),
					                   (const u32*) d_unit_lin, (const u32*) d_unit_off, (const NjFit*) d_fits, (const char*) d_contigs, (const TreeRow*) d_ri,
					                   (const u32*) d_kid, (const u32*) d_par, (const u32*) d_leaf_par, (const u32*) d_rootkid, (const uint8_t*) d_up,
					                   (const u32*) d_active, d_keys, d_cands, (uint8_t*) nullptr, cap_lds);
				}
				if (!lst_slab.empty()) {
					vdjx_prof_scope ps(c, "k_spr_score_slab");
					hipLaunchKernelGGL(k_spr_score<false>, dim3(grid_slab), dim3(64), cap_slab * (SPR_NODE_LDS_BYTES - 64u), st, (const u32*) d_lst_slab,
					                   (u32) lst_slab.size(), (const u32*) d_unit_lin, (const u32*) d_unit_off, (const NjFit*) d_fits, (const char*) d_contigs,
					                   (const TreeRow*) d_ri, (const u32*) d_kid, (const u32*) d_par, (const u32*) d_leaf_par, (const u32*) d_rootkid,
					                   (const uint8_t*) d_up, (const u32*) d_active, d_keys, d_cands, d_slabs, cap_slab);
				}
				{
					vdjx_prof_scope ps(c, "k_spr_pick");
					hipLaunchKernelGGL(k_spr_pick, dim3((u32) which.size()), dim3(SPR_PICK_T), 0, st, (const u32*) d_which, (const NjFit*) d_fits, (const u32*) d_unit_off,
					                   (const char*) d_contigs, (const TreeRow*) d_ri, d_kid, d_par, d_leaf_par, d_rootkid, d_up, d_P, d_active, (const long long*) d_keys,
					                   d_moves, d_rounds, d_still);
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
			HIP_TRY(hipMemcpyAsync(h_cands.data(), d_cands, nl * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
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
					               h_cands[k - k0], (unsigned long long) cand0[big[k]]);
					return VDJX_ESTATE;
				}
				f.root_kid = t.root_kid;                           // (a move can change the root's child: Fitch's passes read it here)
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
				inf.candidates += h_cands[k - k0];
			}
			if (!h_order.empty()) HIP_TRY(hipMemcpyAsync(d_order, h_order.data(), h_order.size() * sizeof(u32), hipMemcpyHostToDevice, st));
			HIP_TRY(hipMemcpyAsync(d_fits, fits.data(), nl * sizeof(NjFit), hipMemcpyHostToDevice, st));
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
		HIP_TRY(hipMemcpyAsync(mut_row.data(), d_mut_row, (size_t) rows * sizeof(u32), hipMemcpyDeviceToHost, st));
		if (inf.internal) HIP_TRY(hipMemcpyAsync(mut_inf.data(), d_mut_inf, (size_t) inf.internal * sizeof(u32), hipMemcpyDeviceToHost, st));
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
		if (inf.parsimony != p_final) {
			vdjx_set_error("%s: the search ended at %llu union events, the final trees have %llu mutations", who, (unsigned long long) p_final,
			               (unsigned long long) inf.parsimony);
			return VDJX_ESTATE;
		}
	}
	if (info) *info = inf;
	c->stats["tree_spr_candidates"] = inf.candidates;
	c->stats["tree_spr_us"] = (u64) std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
	return VDJX_OK;
}
