// vdjx_consensus.hip -- clonal consensus sequences, shazam's collapseClones (gfx950 only, wave64).
//
//   vdjx_consensus_layout   plain C, no GPU: the units, their record, their voters and their column ranges from the hits alone
//   vdjx_consensus          per unit (a group, or a lone contig) and record position the votes of its voters and the winner under a
//                           frequency threshold: the consensus row, the germline row, cover and best (the model: include/vdjx.h; in
//                           Python: tests/consensus_model.py)
//   vdjx_consensus_hits     plain C, no GPU: the rows as pseudo-contigs with V hits, which every consumer of a V hit takes unchanged
//
// The hits are the caller's, checked on the host as vdjx_targeting_counts checks them (vh_check of vdjx_vhit.h) before anything is
// uploaded; the run walk on the device is vh_hit_segments, the one k_tgt_mark and k_sel_counts use.  The host orders the voters by unit (one
// counting sort), deals them to workgroups and cuts the units into batches of whole units of at most VDJX_CONS_CELLS columns.  A batch owns
// six 32-bit counters per column (A, C, G, T, N, gap) in global memory.
//   k_cons_vote     a wave per voter, CONS_WAVES waves per workgroup; a workgroup takes up to CONS_SHARE consecutive voters of ONE unit.
//                   A lane takes every 64th column of the hit, finds its run by bisection in the wave's segment table and votes.  A
//                   workgroup counts in LDS: at most 255 voters, so a counter is a byte and a record position's six counters are two
//                   32-bit words (16 KB for 2,047 positions), added to with 32-bit LDS atomics that cannot carry from byte to byte.  At
//                   the end the non-zero counters go out: with plain stores when the workgroup holds the whole unit, with 32-bit global
//                   atomics when the unit spans several workgroups.  A unit of one voter has nothing to count: up to CONS_WAVES of them
//                   share a workgroup and every vote is a plain store of 1.
//   k_cons_decide   a thread per column of the batch: its unit by bisection over the units' first columns, the six counts, the germline
//                   code -> the two row characters, cover and best.
// No floating point on the device, integer atomics only: they commute, so the result is a function of the multiset of votes -- no order
// of contigs, no batch size and no launch geometry can show.
#include "vdjx_vhit.h"
#include "vdjx_env.h"

#include <chrono>
#include <limits.h>
#include <unordered_map>

#define CONS_WAVES 4
#define CONS_SHARE 255                   // voters per workgroup: what a byte counts
#define CONS_MAXCOLS 2047                // a record's length is below 2,048 (vdjx_germline_load)
#define CONS_SYMS 6                      // A, C, G, T, N, gap

struct ConsVoter {                       // a voter, in unit order
	u32 run_off;                         // its runs in the pool
	u32 nruns;
	u32 contig;                          // its index in the caller's block
	u32 cbase;                           // its unit's first column in the batch
	int seq0;                            // seq_start - 1
	int germ0;                           // germ_start - 1
	int limit;
	int lo;                              // its unit's first record position
};
struct ConsWg {                          // a workgroup's share
	u32 first, count;                    // voters first .. first + count - 1
	u32 mode;                            // 0: lone voters, a wave each; 1: the whole of a unit; 2: a part of a unit
	u32 ncols;                           // the unit's columns (modes 1, 2)
};
struct ConsUnitD { u32 off, rec_at; };   // a unit's first column in its batch; the column of its record position lo in the germline set
static_assert(sizeof(ConsVoter) == 32 && sizeof(ConsWg) == 16 && sizeof(ConsUnitD) == 8, "uploaded as they are");
static_assert(sizeof(vdjx_cons_unit) == 32 && sizeof(vdjx_cons_info) == 80 && sizeof(vdjx_cons_params) == 8, "returned as they are");
static_assert(CONS_SHARE <= 255, "a workgroup's counters are bytes");
static_assert(2 * CONS_MAXCOLS * sizeof(u32) + CONS_WAVES * 64 * sizeof(int4) <= 65536, "within the LDS a kernel may declare");

__global__ __launch_bounds__(64 * CONS_WAVES) void k_cons_vote(const char* __restrict__ contigs, u32 len, const ConsWg* __restrict__ wgs,
                                                              const ConsVoter* __restrict__ vt, const u32* __restrict__ runs,
                                                              u32* __restrict__ cnt) {
	__shared__ int4 seg_all[CONS_WAVES][64];
	__shared__ u32 lc[2 * CONS_MAXCOLS];     // position idx: bytes A C G T in word 2 idx, N gap in word 2 idx + 1
	const u32 tid = threadIdx.x, w = tid >> 6, lane = tid & 63u;
	const ConsWg g = wgs[blockIdx.x];        // (uniform over the workgroup: so are the barriers below)
	if (g.mode != 0) {
		for (u32 i = tid; i < 2 * g.ncols; i += 64 * CONS_WAVES) lc[i] = 0;
		__syncthreads();
	}
	int4* seg = seg_all[w];
	for (u32 k = w; k < g.count; k += CONS_WAVES) {
		const ConsVoter q = vt[g.first + k];
		const char* ct = contigs + (size_t) q.contig * len;
		int tcols, tb, tg;
		seg[lane] = vh_hit_segments(runs, q.run_off, (int) q.nruns, lane, 0, q.seq0, q.germ0, 0, 0, tcols, tb, tg);
		vdjx_wave_lds_fence();               // the table is read by other lanes of the wave
		for (int c = (int) lane; c < tcols; c += 64) {
			int lo = 0, hi = 64;             // the last slot whose first column is <= c: the run that holds c (an empty slot starts at tcols)
			while (hi - lo > 1) {
				const int mid = (lo + hi) >> 1;
				if (seg[mid].x <= c) lo = mid; else hi = mid;
			}
			const int4 s = seg[lo];
			const int op = s.w & 3, off = c - s.x;
			if (op == 1) continue;           // an inserted base has no column
			const int pos = op == 0 ? s.y + off : s.y;      // a deleted position votes while the base after it is below the limit
			if (pos >= q.limit) continue;
			const u32 sym = op == 0 ? (u32) vh_ccode(ct[pos]) : 5u;
			const u32 idx = (u32) (s.z + off - q.lo);       // inside the unit's columns: the host took lo and hi from this walk
			if (g.mode == 0) cnt[(size_t) (q.cbase + idx) * CONS_SYMS + sym] = 1u;
			else atomicAdd(&lc[2u * idx + (sym >> 2)], 1u << (8u * (sym & 3u)));
		}
		vdjx_wave_lds_fence();               // before the next voter's rows replace these
	}
	if (g.mode == 0) return;
	__syncthreads();
	const u32 cbase = vt[g.first].cbase;
	for (u32 i = tid; i < g.ncols; i += 64 * CONS_WAVES) {
		const u32 w0 = lc[2 * i], w1 = lc[2 * i + 1];
		if (!(w0 | w1)) continue;
		u32* out = cnt + (size_t) (cbase + i) * CONS_SYMS;
#pragma unroll
		for (u32 s = 0; s < CONS_SYMS; s++) {
			const u32 v = ((s < 4 ? w0 : w1) >> (8u * (s & 3u))) & 255u;
			if (!v) continue;
			if (g.mode == 1) out[s] = v; else atomicAdd(out + s, v);
		}
	}
}

__global__ __launch_bounds__(256) void k_cons_decide(const ConsUnitD* __restrict__ units, u32 nunits, u32 ncols, const u32* __restrict__ cnt,
                                                    const uint8_t* __restrict__ gcols, u32 num, u32 den, char* __restrict__ cons,
                                                    char* __restrict__ germ, u32* __restrict__ cover, u32* __restrict__ best) {
	const u32 col = blockIdx.x * 256u + threadIdx.x;
	if (col >= ncols) return;
	u32 lo = 0, hi = nunits;                 // the last unit whose first column is <= col (a unit without columns is never the answer)
	while (hi - lo > 1) {
		const u32 mid = (lo + hi) >> 1;
		if (units[mid].off <= col) lo = mid; else hi = mid;
	}
	const ConsUnitD un = units[lo];
	const u32 gb = gcols[un.rec_at + (col - un.off)];
	const uint2* cp = (const uint2*) (cnt + (size_t) col * CONS_SYMS);       // 24 bytes per column: 8-byte aligned
	const uint2 a = cp[0], b = cp[1], d = cp[2];
	const u32 c[CONS_SYMS] = {a.x, a.y, b.x, b.y, d.x, d.y};
	const u32 cv = c[0] + c[1] + c[2] + c[3] + c[4] + c[5];
	const u32 bs = max(max(max(c[0], c[1]), max(c[2], c[3])), c[5]);
	u32 sym = 4;
	if (bs) {
		u32 at = 0, ties = 0;
#pragma unroll
		for (u32 s = 0; s < CONS_SYMS; s++)
			if (s != 4 && c[s] == bs) { at = s; ties++; }
		if (ties == 1) sym = at;
		else if (gb < 4 && c[gb] == bs) sym = gb;
		if ((u64) bs * den < (u64) num * cv) sym = 4;
	}
	cons[col] = "ACGTN-"[sym];
	germ[col] = gb < 4 ? "ACGT"[gb] : 'N';
	cover[col] = cv;
	best[col] = bs;
}

// ---- the host's side -------------------------------------------------------------------------------------------------------------------------
// what the layout alone needs of a usable hit (no record set here): vh_check's list without the record
static int cons_check_hit(const char* who, size_t i, const vdjx_annot_hit& h, int len) {
	int64_t nc, ns, ng;
	if (h.n_runs < 0 || !vh_run_sums(h, nc, ns, ng)) {
		vdjx_set_error("%s: contig %zu: the V hit has a run with an op outside 0..2 or a length of 0 (n_runs %d)", who, i, h.n_runs);
		return VDJX_EINVAL;
	}
	if (h.seq_start < 1 || h.germ_start < 1 || h.seq_end > len || h.germ_end > CONS_MAXCOLS) {
		vdjx_set_error("%s: contig %zu: the V hit's contig positions %d .. %d (1 .. %d) or germline positions %d .. %d (1 .. %d)", who, i,
		               h.seq_start, h.seq_end, len, h.germ_start, h.germ_end, CONS_MAXCOLS);
		return VDJX_EINVAL;
	}
	if (ns != (int64_t) h.seq_end - h.seq_start + 1 || ng != (int64_t) h.germ_end - h.germ_start + 1) {
		vdjx_set_error("%s: contig %zu: the V hit's runs hold %lld contig and %lld germline bases, its positions %d .. %d and %d .. %d", who, i,
		               (long long) ns, (long long) ng, h.seq_start, h.seq_end, h.germ_start, h.germ_end);
		return VDJX_EINVAL;
	}
	return VDJX_OK;
}

struct ConsTotals { u64 used = 0, truncated = 0, off_record = 0, inserted = 0, columns = 0; };

// the units, in the order of their first usable contig; out_unit[i]: the voter's unit or -1
static int cons_layout(const char* who, const vdjx_annot_hit* v, const int32_t* limit, const int32_t* group, size_t n, int len, int32_t* out_unit,
                       std::vector<vdjx_cons_unit>& units, ConsTotals& tot) {
	std::unordered_map<int32_t, u32> of_group;
	std::vector<std::pair<u64, u32>> named;      // (unit << 32 | record, contig) of every usable contig
	units.clear();
	for (size_t i = 0; i < n; i++) {
		out_unit[i] = -1;
		const int lim = limit ? limit[i] : len;
		if (lim < 0 || lim > len) { vdjx_set_error("%s: contig %zu: limit %d (0 .. %d)", who, i, lim, len); return VDJX_EINVAL; }
		if (vh_called(v[i]) && !vh_usable(v[i])) { tot.truncated++; continue; }
		if (!vh_usable(v[i])) continue;
		const int rc = cons_check_hit(who, i, v[i], len);
		if (rc != VDJX_OK) return rc;
		tot.used++;
		u32 u;
		const bool lone = !group || group[i] < 0;
		const auto it = lone ? of_group.end() : of_group.find(group[i]);
		if (it != of_group.end()) u = it->second;
		else {
			u = (u32) units.size();
			vdjx_cons_unit nu;
			memset(&nu, 0, sizeof nu);
			nu.group = lone ? -1 : group[i];
			nu.gene = -1;
			nu.lo = INT_MAX;
			units.push_back(nu);
			if (!lone) of_group.emplace(group[i], u);
		}
		named.push_back({(u64) u << 32 | (u32) v[i].gene, (u32) i});
	}
	// a unit's record: the one most of its usable contigs name, the lowest index on a tie (the pairs ascend by record inside a unit)
	std::sort(named.begin(), named.end());
	std::vector<u32> most(units.size(), 0);
	for (size_t a = 0; a < named.size();) {
		size_t b = a;
		while (b < named.size() && named[b].first == named[a].first) b++;
		const u32 u = (u32) (named[a].first >> 32);
		if ((u32) (b - a) > most[u]) { most[u] = (u32) (b - a); units[u].gene = (int32_t) (u32) named[a].first; }
		a = b;
	}
	for (const auto& e : named) {
		const u32 u = (u32) (e.first >> 32), i = e.second;
		vdjx_cons_unit& un = units[u];
		if (v[i].gene != un.gene) { un.off_record++; tot.off_record++; continue; }
		out_unit[i] = (int32_t) u;
		un.members++;
		// the voter's walk: where it votes, and its inserted bases below the limit
		const int lim = limit ? limit[i] : len;
		int q = v[i].seq_start - 1, p = v[i].germ_start - 1;
		for (int r = 0; r < v[i].n_runs; r++) {
			const int L = (int) (v[i].runs[r] >> 4), op = (int) (v[i].runs[r] & 15u);
			const int below = std::max(0, std::min(L, lim - q));
			const int voted = op == 0 ? below : op == 2 && q < lim ? L : 0;
			if (voted) {
				un.lo = std::min(un.lo, p);
				un.hi = std::max(un.hi, p + voted);
			}
			if (op == 1) tot.inserted += (u64) below;
			if (op != 2) q += L;
			if (op != 1) p += L;
		}
	}
	u64 off = 0;
	for (vdjx_cons_unit& un : units) {
		if (un.lo == INT_MAX) un.lo = un.hi = 0;
		un.off = off;
		off += (u64) (un.hi - un.lo);
	}
	tot.columns = off;
	return VDJX_OK;
}

extern "C" int vdjx_consensus_layout(const vdjx_annot_hit* v, const int32_t* limit, const int32_t* group, size_t n, int len, int32_t* out_unit,
                                     vdjx_cons_unit* out_units, uint64_t* n_units, uint64_t* n_cols) {
	if (n_units) *n_units = 0;
	if (n_cols) *n_cols = 0;
	if (!n_units || !n_cols) { vdjx_set_error("vdjx_consensus_layout: NULL argument"); return VDJX_EINVAL; }
	if (n == 0) return VDJX_OK;
	if (!v || !out_unit || !out_units) { vdjx_set_error("vdjx_consensus_layout: NULL argument"); return VDJX_EINVAL; }
	int rc = vh_check_sizes("vdjx_consensus_layout", n, len);
	if (rc != VDJX_OK) return rc;
	std::vector<vdjx_cons_unit> units;
	ConsTotals tot;
	rc = cons_layout("vdjx_consensus_layout", v, limit, group, n, len, out_unit, units, tot);
	if (rc != VDJX_OK) return rc;
	if (!units.empty()) memcpy(out_units, units.data(), units.size() * sizeof(vdjx_cons_unit));
	*n_units = units.size();
	*n_cols = tot.columns;
	return VDJX_OK;
}

extern "C" int vdjx_consensus(vdjx_ctx* c, const char* contigs, size_t n, int len, const vdjx_annot_hit* v, const int32_t* limit,
                              const int32_t* group, const vdjx_cons_params* params, char* out_cons, char* out_germ, uint32_t* out_cover,
                              uint32_t* out_best, vdjx_cons_unit* out_units, int32_t* out_unit, vdjx_cons_info* info) {
	if (info) memset(info, 0, sizeof *info);
	if (!c) { vdjx_set_error("vdjx_consensus: NULL argument"); return VDJX_EINVAL; }
	if (n == 0) return VDJX_OK;
	if (!contigs || !v || !out_cons || !out_germ || !out_units || !out_unit) { vdjx_set_error("vdjx_consensus: NULL argument"); return VDJX_EINVAL; }
	const vdjx_cons_params prm = params ? *params : vdjx_cons_params{6000, 10000};
	if (prm.den < 1 || prm.den > 1000000 || prm.num < 0 || prm.num > prm.den) {
		vdjx_set_error("vdjx_consensus: the minimum share %d / %d (den 1 .. 10^6, num 0 .. den)", prm.num, prm.den);
		return VDJX_EINVAL;
	}
	int rc = vh_check_sizes("vdjx_consensus", n, len);
	if (rc != VDJX_OK) return rc;
	rc = vh_check_contigs("vdjx_consensus", c, contigs, n, len);
	if (rc != VDJX_OK) return rc;
	const vdjx_recset& gs = c->germline;
	const u64 cells = (u64) vdjx_env_num("VDJX_CONS_CELLS", 1 << 24, 1, 1 << 28);
	const auto t0 = std::chrono::steady_clock::now();
	std::vector<size_t> slot(n, 0);
	for (size_t i = 0; i < n; i++) {
		const int lim = limit ? limit[i] : len;
		if (lim < 0 || lim > len) { vdjx_set_error("vdjx_consensus: contig %zu: limit %d (0 .. %d)", i, lim, len); return VDJX_EINVAL; }
		if (!vh_usable(v[i])) continue;
		rc = vh_check("vdjx_consensus", "V", i, v[i], gs, 0, len, &slot[i]);
		if (rc != VDJX_OK) return rc;
	}
	std::vector<vdjx_cons_unit> units;
	ConsTotals tot;
	rc = cons_layout("vdjx_consensus", v, limit, group, n, len, out_unit, units, tot);
	if (rc != VDJX_OK) return rc;
	const size_t U = units.size();

	// the batches: whole units, at most `cells` columns (a unit of more is a batch of its own); boff[b]: its first unit, one more entry: U
	std::vector<u32> bfirst;
	std::vector<u64> bcol;                   // the batch's first column in the caller's rows
	std::vector<u32> ubatch(U);
	{
		u64 held = 0;
		for (size_t u = 0; u < U; u++) {
			const u64 w = (u64) (units[u].hi - units[u].lo);
			if (u == 0 || held + w > cells) { bfirst.push_back((u32) u); bcol.push_back(units[u].off); held = 0; }
			held += w;
			ubatch[u] = (u32) bfirst.size() - 1;
		}
		bfirst.push_back((u32) U);
		bcol.push_back(tot.columns);
	}
	const u32 batches = (u32) bfirst.size() - 1;
	u64 cap = 0;
	for (u32 b = 0; b < batches; b++) cap = std::max(cap, bcol[b + 1] - bcol[b]);

	// the voters by unit: one counting sort (the members are the counts), contig order inside a unit
	std::vector<u32> vfirst(U + 1, 0);
	for (size_t u = 0; u < U; u++) vfirst[u + 1] = vfirst[u] + units[u].members;
	const u32 voters = vfirst[U];
	std::vector<ConsVoter> vt(voters);
	std::vector<ConsUnitD> du(U);
	std::vector<u32> runs;
	{
		std::vector<u32> fill(vfirst.begin(), vfirst.end() - 1);
		for (size_t i = 0; i < n; i++) {
			if (out_unit[i] < 0) continue;
			const u32 u = (u32) out_unit[i];
			ConsVoter q;
			q.run_off = (u32) runs.size();
			q.nruns = (u32) v[i].n_runs;
			runs.insert(runs.end(), v[i].runs, v[i].runs + q.nruns);
			q.contig = (u32) i;
			q.cbase = (u32) (units[u].off - bcol[ubatch[u]]);
			q.seq0 = v[i].seq_start - 1;
			q.germ0 = v[i].germ_start - 1;
			q.limit = limit ? limit[i] : len;
			q.lo = units[u].lo;
			vt[fill[u]++] = q;
			du[u].off = q.cbase;
			du[u].rec_at = (u32) (gs.at[0][slot[i]] + 1 + (u64) units[u].lo);      // (every voter of a unit names the same record)
		}
	}
	// the workgroups: lone voters CONS_WAVES at a time, a unit's voters CONS_SHARE at a time; never across a batch
	std::vector<ConsWg> wgs;
	std::vector<u32> wfirst(batches + 1, 0);
	u32 large = 0;
	for (u32 b = 0; b < batches; b++) {
		wfirst[b] = (u32) wgs.size();
		for (u32 u = bfirst[b]; u < bfirst[b + 1]; u++) {
			const u32 m = units[u].members, nc = (u32) (units[u].hi - units[u].lo);
			if (nc == 0) continue;           // nobody voted
			if (m == 1) {
				if (!wgs.empty() && wgs.back().mode == 0 && wgs.back().count < CONS_WAVES && wgs.size() > wfirst[b] &&
				    wgs.back().first + wgs.back().count == vfirst[u]) wgs.back().count++;
				else wgs.push_back({vfirst[u], 1, 0, 0});
				continue;
			}
			if (m > CONS_SHARE) large++;
			for (u32 a = 0; a < m; a += CONS_SHARE) wgs.push_back({vfirst[u] + a, std::min<u32>(CONS_SHARE, m - a), m > CONS_SHARE ? 2u : 1u, nc});
		}
	}
	wfirst[batches] = (u32) wgs.size();

	std::vector<char> h_cons(tot.columns ? tot.columns : 1), h_germ(tot.columns ? tot.columns : 1);
	std::vector<u32> h_cover, h_best;
	u32* cover = out_cover;
	if (!cover) { h_cover.resize(tot.columns ? tot.columns : 1); cover = h_cover.data(); }
	if (tot.columns) {
		HIP_TRY(hipSetDevice(c->device));
		hipStream_t st = c->stream;
		vdjx_work wk(c);
		char *d_ct, *d_cons, *d_germ;
		ConsVoter* d_vt;
		ConsWg* d_wg;
		ConsUnitD* d_units;
		u32 *d_runs, *d_cnt, *d_cover, *d_best;
		HIP_TRY(wk.alloc(&d_ct, n * (size_t) len));
		HIP_TRY(wk.alloc(&d_vt, (size_t) voters));
		HIP_TRY(wk.alloc(&d_wg, wgs.size()));
		HIP_TRY(wk.alloc(&d_units, U));
		HIP_TRY(wk.alloc(&d_runs, runs.size()));
		HIP_TRY(wk.alloc(&d_cnt, (size_t) cap * CONS_SYMS));
		HIP_TRY(wk.alloc(&d_cover, (size_t) cap));
		HIP_TRY(wk.alloc(&d_best, (size_t) cap));
		HIP_TRY(wk.alloc(&d_cons, (size_t) cap));
		HIP_TRY(wk.alloc(&d_germ, (size_t) cap));
		HIP_TRY(hipMemcpyAsync(d_ct, contigs, n * (size_t) len, hipMemcpyHostToDevice, st));
		HIP_TRY(hipMemcpyAsync(d_vt, vt.data(), (size_t) voters * sizeof(ConsVoter), hipMemcpyHostToDevice, st));
		HIP_TRY(hipMemcpyAsync(d_wg, wgs.data(), wgs.size() * sizeof(ConsWg), hipMemcpyHostToDevice, st));
		HIP_TRY(hipMemcpyAsync(d_units, du.data(), U * sizeof(ConsUnitD), hipMemcpyHostToDevice, st));
		if (!runs.empty()) HIP_TRY(hipMemcpyAsync(d_runs, runs.data(), runs.size() * sizeof(u32), hipMemcpyHostToDevice, st));
		for (u32 b = 0; b < batches; b++) {
			const u64 nc = bcol[b + 1] - bcol[b];
			const u32 nw = wfirst[b + 1] - wfirst[b], nu = bfirst[b + 1] - bfirst[b];
			if (nc == 0) continue;
			HIP_TRY(hipMemsetAsync(d_cnt, 0, (size_t) nc * CONS_SYMS * sizeof(u32), st));
			{
				vdjx_prof_scope ps(c, "k_cons_vote");
				hipLaunchKernelGGL(k_cons_vote, dim3(nw), dim3(64 * CONS_WAVES), 0, st, (const char*) d_ct, (u32) len, (const ConsWg*) d_wg + wfirst[b],
				                   (const ConsVoter*) d_vt, (const u32*) d_runs, d_cnt);
			}
			{
				vdjx_prof_scope ps(c, "k_cons_decide");
				hipLaunchKernelGGL(k_cons_decide, dim3((u32) ((nc + 255) / 256)), dim3(256), 0, st, (const ConsUnitD*) d_units + bfirst[b], nu, (u32) nc,
				                   (const u32*) d_cnt, (const uint8_t*) c->germline.d_cols, (u32) prm.num, (u32) prm.den, d_cons, d_germ, d_cover, d_best);
			}
			HIP_TRY(hipMemcpyAsync(h_cons.data() + bcol[b], d_cons, (size_t) nc, hipMemcpyDeviceToHost, st));
			HIP_TRY(hipMemcpyAsync(h_germ.data() + bcol[b], d_germ, (size_t) nc, hipMemcpyDeviceToHost, st));
			HIP_TRY(hipMemcpyAsync(cover + bcol[b], d_cover, (size_t) nc * sizeof(u32), hipMemcpyDeviceToHost, st));
			if (out_best) HIP_TRY(hipMemcpyAsync(out_best + bcol[b], d_best, (size_t) nc * sizeof(u32), hipMemcpyDeviceToHost, st));
			HIP_TRY(hipStreamSynchronize(st));       // (the next batch reuses the buffers, and the copies land in pageable memory)
		}
		HIP_TRY(hipGetLastError());
		vdjx_prof_collect(c, false);
		memcpy(out_cons, h_cons.data(), tot.columns);
		memcpy(out_germ, h_germ.data(), tot.columns);
	}
	if (U) memcpy(out_units, units.data(), U * sizeof(vdjx_cons_unit));
	u64 votes = 0, undecided = 0;
	for (u64 k = 0; k < tot.columns; k++) {
		votes += cover[k];
		undecided += h_cons[k] == 'N' && cover[k] > 0;
	}
	if (info) {
		info->contigs = n;
		info->used = tot.used;
		info->truncated = tot.truncated;
		info->off_record = tot.off_record;
		info->units = U;
		info->columns = tot.columns;
		info->votes = votes;
		info->inserted = tot.inserted;
		info->undecided = undecided;
		info->batches = tot.columns ? batches : 0;
		info->large_units = large;
	}
	c->stats["consensus_units"] = U;
	c->stats["consensus_batches"] = tot.columns ? batches : 0;
	c->stats["consensus_us"] = (u64) std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
	return VDJX_OK;
}

// plain C, no GPU: a unit's rows -> its pseudo-contig and the V hit that lays it against the unit's record
extern "C" int vdjx_consensus_hits(const vdjx_cons_unit* units, size_t U, const char* cons, const char* germ, int plen, char* out_contigs,
                                   vdjx_annot_hit* out_hits, int* out_plen) {
	if (!out_plen) { vdjx_set_error("vdjx_consensus_hits: NULL argument"); return VDJX_EINVAL; }
	*out_plen = 1;
	if (U == 0) return VDJX_OK;
	if (!units || !cons || !germ) { vdjx_set_error("vdjx_consensus_hits: NULL argument"); return VDJX_EINVAL; }
	int longest = 1;
	for (size_t u = 0; u < U; u++) {
		if (units[u].hi < units[u].lo || units[u].lo < 0 || units[u].hi > CONS_MAXCOLS) {
			vdjx_set_error("vdjx_consensus_hits: unit %zu: positions %d .. %d (0 .. %d)", u, units[u].lo, units[u].hi, CONS_MAXCOLS);
			return VDJX_EINVAL;
		}
		int bases = 0;
		for (int k = 0; k < units[u].hi - units[u].lo; k++) bases += cons[units[u].off + (u64) k] != '-';
		longest = std::max(longest, bases);
	}
	*out_plen = longest;
	if (!out_contigs) return VDJX_OK;
	if (!out_hits) { vdjx_set_error("vdjx_consensus_hits: NULL argument"); return VDJX_EINVAL; }
	if (plen < longest || plen >= 4096) {
		vdjx_set_error("vdjx_consensus_hits: plen %d (the longest row has %d bases; at most 4095)", plen, longest);
		return VDJX_EINVAL;
	}
	memset(out_contigs, 'N', U * (size_t) plen);
	for (size_t u = 0; u < U; u++) {
		const char *cr = cons + units[u].off, *gr = germ + units[u].off;
		vdjx_annot_hit& h = out_hits[u];
		memset(&h, 0, sizeof h);
		h.gene = -1;
		for (int z = 0; z < VDJX_ANNOT_TIED; z++) h.tied[z] = -1;
		int a = 0, b = units[u].hi - units[u].lo;        // the columns between the gap columns at either end
		while (a < b && cr[a] == '-') a++;
		while (b > a && cr[b - 1] == '-') b--;
		if (a == b) continue;                // no base: no hit
		char* pc = out_contigs + u * (size_t) plen;
		int nb = 0;
		for (int k = a; k < b;) {
			const bool gap = cr[k] == '-';
			int e = k;
			while (e < b && (cr[e] == '-') == gap) e++;
			for (int x = k; x < e; x++) {
				if (gap) { h.del++; continue; }
				pc[nb++] = cr[x];
				const bool acgt = cr[x] == 'A' || cr[x] == 'C' || cr[x] == 'G' || cr[x] == 'T';
				if (acgt && cr[x] == gr[x]) h.matches++; else h.mismatches++;
			}
			if (gap) h.opens++;
			if (h.n_runs < VDJX_ANNOT_RUNS) h.runs[h.n_runs] = (u32) (e - k) << 4 | (gap ? 2u : 0u);
			h.n_runs++;
			k = e;
		}
		if (h.n_runs > VDJX_ANNOT_RUNS) memset(h.runs, 0, sizeof h.runs);      // (as vdjx_annotate: the count is kept, there are no runs to read)
		h.gene = units[u].gene;
		h.score = std::max(1, h.matches);
		h.n_tied = 1;
		h.tied[0] = h.gene;
		h.seq_start = 1;
		h.seq_end = nb;
		h.germ_start = units[u].lo + a + 1;
		h.germ_end = units[u].lo + b;
	}
	return VDJX_OK;
}
