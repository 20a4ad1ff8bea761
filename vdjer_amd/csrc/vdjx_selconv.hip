// vdjx_selconv.hip -- BASELINe's group posteriors: the members' own posteriors of sigma, convolved (gfx950 only, wave64).
//
//   vdjx_selection_convolve   per row (a group, or all contigs) and region the distribution of the mean of the contributing members'
//                             independent sigmas on vdjx_selection's grid (the model: include/vdjx.h; in Python:
//                             tests/selection_conv_model.py)
//
// The counts are vdjx_selection's; a member is formed from its count row by the code vdjx_selection uses (sel_member of vdjx_selpost.h) and
// the groups are ordered by its counting sort (sel_group_order).  The host lays out the whole call as a list of launches before the first
// one: the tree of a row depends only on its number of leaves, so nothing comes back from the device in between.
//   k_conv_leaf      a workgroup per leaf: l[T] in LDS from the member's terms (sel_terms) plus the prior, the block maximum,
//                    f = exp(l - max), the block sum S; the mass f / S to the leaf's cell.  A row without a contributing member has one
//                    leaf, the prior.
//   k_conv_combine   one launch per level of the rows in flight; a workgroup per (job, tile of 256 output cells).  The left density A
//                    (32 KB) and the right one (35 KB) in LDS, two workgroups per CU.  A thread owns one output cell and GATHERS its terms
//                    into a register, so there are no atomics and the order of a cell's sum is the loop's.
//                    a = b:  C[w] = sum_u A[u] B'[2w - u], B'[s] = B[s - 1] / 2 + B[s] + B[s + 1] / 2 (s = -2001 .. 2001).  B' is formed once
//                            per workgroup and stored by parity -- even s in one array, odd s in another -- because at a fixed u the lanes
//                            read s = 2w - u, every second entry: split by parity the 64 lanes of a wave read 64 neighbouring doubles (no
//                            bank conflict) where the interleaved array would put lanes l and l + 16 on one bank.  u runs ascending in
//                            pairs (2p, 2p + 1), 32 pairs to a chunk: the wave reads the chunk's 64 values of A with one LDS read, a lane
//                            each, and every step takes its two from their lanes into scalar registers (v_readlane), so that a step's LDS
//                            traffic is the two reads of B' alone (a broadcast read of A per step made the loop 1.4 times slower).  A wave
//                            walks only the p that one of its cells needs; 96 zeros on either side of both arrays stand for the entries a
//                            neighbouring lane's cell does not have and for the steps of a last chunk past the wave's last pair, whose A
//                            is 0.
//                    a > b:  v ascending over the right density; the left one's u with |a u + b v - c (a + b)| < a + b are among six
//                            neighbours of (c (a + b) - b v) / a, u ascending, each with the share max(0, den - |a u + b v - c den|) / den
//                            (0 outside the grid).  The integers are exact in float64.  At most one job per level of a row comes here.
//   k_conv_finish    a workgroup per finished row: the root's cell through sel_finish_tail (vdjx_selpost.h), k_sel_finish's rules.
// Every cell is written by one thread in one launch and read only by later launches of the stream.
#include "vdjx_selpost.h"
#include "vdjx_env.h"

#include <string.h>

#include <algorithm>
#include <chrono>
#include <vector>

#define CV_TILES 16                      // tiles of 256 output cells: 4096 >= 4001
#define CV_STEP 32                       // pairs of A per chunk: a wave's 64 lanes hold them
#define CV_PAD 96                        // 64 for the neighbouring lanes' cells, 32 for the steps past a wave's last pair (their A is 0)
#define CV_HALF 2196                     // one parity class of B': entries -96 .. 2099
#define CV_A 4008                        // A and zeros behind it (A[4001]: the partner of A[4000] in the last pair)

struct ConvJob { u32 left, right, out, a, b, pad; };   // cells and weights: (left, a) (+) (right, b) -> (out, a + b), a >= b
struct ConvFin { u32 cell, out; };                     // the root's cell -> out_stat[out], out_pdf[out]
static_assert(sizeof(ConvJob) == 24 && sizeof(ConvFin) == 8 && sizeof(vdjx_selconv_info) == 48, "uploaded / returned as they are");

__global__ __launch_bounds__(256) void k_conv_leaf(const SelMember* __restrict__ members, const u32* __restrict__ cell, double* __restrict__ cells) {
	__shared__ double ell[SEL_T];
	__shared__ double red[4];
	const u32 tid = threadIdx.x;
	const SelMember* m = members + blockIdx.x;
	double mx = -INFINITY;
	for (int t = (int) tid; t < SEL_T; t += 256) {
		const double sg = sel_sigma(t);
		double l = sg - 2.0 * sel_softplus(sg);
		l += sel_terms(m, 1, sg);
		ell[t] = l;
		mx = fmax(mx, l);
	}
	mx = sel_block_max(mx, red);         // (its barriers publish ell)
	const int t0 = (int) tid * SEL_PER;
	double f[SEL_PER];
	double loc = 0.0;
#pragma unroll
	for (int j = 0; j < SEL_PER; j++) {
		f[j] = t0 + j < SEL_T ? exp(ell[t0 + j] - mx) : 0.0;
		loc += f[j];
	}
	const double S = sel_block_sum(loc, red);        // (its barriers: every thread has read its ell)
#pragma unroll
	for (int j = 0; j < SEL_PER; j++)
		if (t0 + j < SEL_T) ell[t0 + j] = f[j] / S;
	__syncthreads();
	double* o = cells + (size_t) cell[blockIdx.x] * SEL_T;
	for (int t = (int) tid; t < SEL_T; t += 256) o[t] = ell[t];
}

// B'[j] of the right density, j = s + 2000 = -1 .. 4001
__device__ __forceinline__ double conv_bprime(const double* __restrict__ B, int j) {
	const double lo = j >= 1 && j <= SEL_T ? B[j - 1] : 0.0;
	const double mid = j >= 0 && j < SEL_T ? B[j] : 0.0;
	const double hi = j >= -1 && j < SEL_T - 1 ? B[j + 1] : 0.0;
	return (0.5 * lo + mid) + 0.5 * hi;
}

// lane `from`'s value in every lane, through scalar registers (from: a constant)
__device__ __forceinline__ double conv_lane(double v, int from) {
	const long long b = __double_as_longlong(v);
	const u32 lo = (u32) __builtin_amdgcn_readlane((int) (u32) b, from), hi = (u32) __builtin_amdgcn_readlane((int) (u32) ((u64) b >> 32), from);
	return __longlong_as_double((long long) ((u64) hi << 32 | lo));
}

__global__ __launch_bounds__(256) void k_conv_combine(double* __restrict__ cells, const ConvJob* __restrict__ jobs) {
	__shared__ __attribute__((aligned(16))) double sA[CV_A];
	__shared__ __attribute__((aligned(16))) double sB[2 * CV_HALF];
	const ConvJob jb = jobs[blockIdx.x / CV_TILES];
	const u32 tile = blockIdx.x % CV_TILES, tid = threadIdx.x;
	const double* A = cells + (size_t) jb.left * SEL_T;
	const double* B = cells + (size_t) jb.right * SEL_T;
	const int k = (int) (tile * 256 + tid);          // the output cell, c = k - 2000
	for (int t = (int) tid; t < CV_A; t += 256) sA[t] = t < SEL_T ? A[t] : 0.0;
	double acc = 0.0;
	if (jb.a == jb.b) {
		for (int x = (int) tid; x < 2 * CV_HALF; x += 256) {
			const int par = x >= CV_HALF;
			const int j = 2 * (x - par * CV_HALF - CV_PAD) + par;
			sB[x] = j >= -1 && j <= SEL_T ? conv_bprime(B, j) : 0.0;
		}
		__syncthreads();
		// u = i - 2000, i = 2p and 2p + 1: B' at j = 2k - i, entry k - p of the even class and k - p - 1 of the odd one
		const int k0 = (int) (tile * 256 + (tid & ~63u));
		const int p_lo = __builtin_amdgcn_readfirstlane(max(0, k0 - 2001)), p_hi = __builtin_amdgcn_readfirstlane(min(2000, k0 + 63));
		const double* be = sB + CV_PAD + k;
		const double* bo = sB + CV_HALF + CV_PAD + k - 1;
		// 32 pairs at a time: lane j takes A[2p + j] (0 past the wave's last pair), every step reads its two values from their lanes into
		// scalar registers, so that a step's LDS traffic is the two B' reads alone
		const int lane = (int) (tid & 63u);
		for (int pb = p_lo; pb <= p_hi; pb += CV_STEP) {
			const int ai = 2 * pb + lane;
			const double av = ai <= 2 * p_hi + 1 ? sA[ai] : 0.0;
#pragma unroll
			for (int i = 0; i < CV_STEP; i++) {
				acc = fma(conv_lane(av, 2 * i), be[-(pb + i)], acc);
				acc = fma(conv_lane(av, 2 * i + 1), bo[-(pb + i)], acc);
			}
		}
	} else {
		for (int t = (int) tid; t < 2 * CV_HALF; t += 256) sB[t] = t < SEL_T ? B[t] : 0.0;
		__syncthreads();
		const double a = (double) jb.a, b = (double) jb.b, den = a + b, ra = 1.0 / a, rden = 1.0 / den;
		const double cd = (double) (k - 2000) * den;
		for (int v = 0; v < SEL_T; v++) {
			const double bv = sB[v];
			const double rest = cd - b * (double) (v - 2000);      // a u lies within den of it
			const int u0 = (int) floor(rest * ra) - 2;
#pragma unroll
			for (int e = 0; e < 6; e++) {
				const int u = u0 + e;
				const double share = fmax(den - fabs(a * (double) u - rest), 0.0) * rden;
				const int ui = u + 2000;
				const double av = sA[(unsigned) ui <= 4000u ? ui : SEL_T];      // (sA[4001] = 0)
				acc += (av * bv) * share;
			}
		}
	}
	if (k < SEL_T) cells[(size_t) jb.out * SEL_T + (size_t) k] = acc;
}

__global__ __launch_bounds__(256) void k_conv_finish(const double* __restrict__ cells, const ConvFin* __restrict__ fins, const vdjx_sel_stat* __restrict__ head,
                                                     vdjx_sel_stat* __restrict__ out_stat, double* __restrict__ out_pdf) {
	__shared__ double ell[SEL_T];
	__shared__ double tot[256];
	__shared__ double red[4];
	__shared__ int qidx[2][4];
	const ConvFin fj = fins[blockIdx.x];
	const u32 tid = threadIdx.x;
	const double* C = cells + (size_t) fj.cell * SEL_T;
	for (int t = (int) tid; t < SEL_T; t += 256) ell[t] = C[t];
	__syncthreads();
	const int t0 = (int) tid * SEL_PER;
	double f[SEL_PER];
#pragma unroll
	for (int j = 0; j < SEL_PER; j++) f[j] = t0 + j < SEL_T ? ell[t0 + j] : 0.0;
	const vdjx_sel_stat* h = head + fj.out;
	sel_finish_tail(f, ell, tot, red, qidx, h->sequences, h->x, h->n, h->exp_r, h->exp_s, out_stat + fj.out, out_pdf ? out_pdf + (size_t) fj.out * SEL_T : nullptr);
}

// ---- the host's side -------------------------------------------------------------------------------------------------------------------------
namespace {
struct ConvEntry { u32 cell, w; };
struct ConvOp { u32 kind, start, count; };               // 0 leaves, 1 combines, 2 finishes: a launch over [start, start + count) of its list
struct ConvPlan {
	std::vector<SelMember> leaf_m;
	std::vector<u32> leaf_cell;
	std::vector<ConvJob> jobs;
	std::vector<ConvFin> fins;
	std::vector<ConvOp> ops;
	std::vector<u32> freec;
	u32 ncell = 0, batches = 0;
	u32 take() {
		if (freec.empty()) return ncell++;
		const u32 c = freec.back();
		freec.pop_back();
		return c;
	}
	void give(u32 c) { freec.push_back(c); }
	ConvEntry combine(ConvEntry l, ConvEntry r) {        // (the caller gives the inputs' cells back once the launch is laid out)
		const u32 o = take();
		jobs.push_back({l.cell, r.cell, o, l.w, r.w, 0u});
		return {o, l.w + r.w};
	}
	// the trees of several runs of leaves at once, level by level: adjacent pairs, an odd last entry passes through
	void reduce(const std::vector<std::pair<const SelMember*, u32>>& runs, std::vector<ConvEntry>& roots) {
		batches++;
		std::vector<std::vector<ConvEntry>> ent(runs.size());
		const u32 l0 = (u32) leaf_m.size();
		for (size_t r = 0; r < runs.size(); r++)
			for (u32 a = 0; a < runs[r].second; a++) {
				const u32 c = take();
				leaf_m.push_back(runs[r].first[a]);
				leaf_cell.push_back(c);
				ent[r].push_back({c, 1u});
			}
		ops.push_back({0u, l0, (u32) leaf_m.size() - l0});
		for (;;) {
			const u32 j0 = (u32) jobs.size();
			for (auto& e : ent) {
				if (e.size() < 2) continue;
				std::vector<ConvEntry> nx;
				for (size_t a = 0; a + 1 < e.size(); a += 2) nx.push_back(combine(e[a], e[a + 1]));
				if (e.size() & 1) nx.push_back(e.back());
				e.swap(nx);
			}
			if (jobs.size() == j0) break;
			ops.push_back({1u, j0, (u32) jobs.size() - j0});
			for (size_t a = j0; a < jobs.size(); a++) { give(jobs[a].left); give(jobs[a].right); }
		}
		roots.clear();
		for (auto& e : ent) roots.push_back(e[0]);
	}
	ConvEntry single(ConvEntry l, ConvEntry r) {         // one combination as a launch of its own (a streamed row's stack)
		const u32 j0 = (u32) jobs.size();
		const ConvEntry o = combine(l, r);
		ops.push_back({1u, j0, 1u});
		give(l.cell); give(r.cell);
		return o;
	}
	void finish(const std::vector<ConvEntry>& roots, const std::vector<u32>& outs) {
		const u32 f0 = (u32) fins.size();
		for (size_t a = 0; a < roots.size(); a++) { fins.push_back({roots[a].cell, outs[a]}); give(roots[a].cell); }
		if (fins.size() > f0) ops.push_back({2u, f0, (u32) fins.size() - f0});
	}
};
u32 conv_log2_up(u32 m) { u32 l = 0; while ((1u << l) < m) l++; return l; }
}

extern "C" int vdjx_selection_convolve(vdjx_ctx* c, const vdjx_sel_counts* counts, size_t n, uint32_t K, const int32_t* group, uint32_t G,
                                       vdjx_sel_stat* out_stat, double* out_pdf, vdjx_selconv_info* info) {
	if (info) memset(info, 0, sizeof *info);
	if (!c) { vdjx_set_error("vdjx_selection_convolve: NULL argument"); return VDJX_EINVAL; }
	if (n == 0) return VDJX_OK;
	if (!counts || !out_stat) { vdjx_set_error("vdjx_selection_convolve: NULL argument"); return VDJX_EINVAL; }
	if (K < 1 || K > 2) { vdjx_set_error("vdjx_selection_convolve: %u regions (1 or 2)", K); return VDJX_EINVAL; }
	if (G >= (1u << 20)) { vdjx_set_error("vdjx_selection_convolve: %u groups (at most 2^20 - 1)", G); return VDJX_EINVAL; }
	if (n >= ((size_t) 1 << 20)) { vdjx_set_error("vdjx_selection_convolve: %zu contigs (at most 2^20 - 1)", n); return VDJX_EINVAL; }
	if (G && !group) { vdjx_set_error("vdjx_selection_convolve: %u groups and no group array", G); return VDJX_EINVAL; }
	if (out_pdf && (u64) G + 1 > 65536) { vdjx_set_error("vdjx_selection_convolve: densities of %u groups and the sample (at most 65536 rows)", G); return VDJX_EINVAL; }
	if (G)
		for (size_t i = 0; i < n; i++)
			if (group[i] >= 0 && (u32) group[i] >= G) { vdjx_set_error("vdjx_selection_convolve: contig %zu: group %d of %u", i, group[i], G); return VDJX_EINVAL; }
	const u64 cap = (u64) vdjx_env_num("VDJX_CONV_CELLS", 1 << 15, 4, 1 << 20);
	const auto t0 = std::chrono::steady_clock::now();

	// the rows' contributing members, per (row, region) in contig order, and the heads of their stats
	std::vector<u32> gstart, gorder;
	sel_group_order(group, n, G, gstart, gorder);
	const size_t R = (size_t) G + 1, NR = R * K;
	std::vector<vdjx_sel_stat> head(NR);
	std::vector<SelMember> mem;                          // every row's leaves, one row and region after the other
	std::vector<size_t> mstart(NR + 1, 0);
	u64 members = 0;
	for (size_t r = 0; r < R; r++)
		for (u32 k = 0; k < K; k++) {
			vdjx_sel_stat& h = head[r * K + k];
			memset(&h, 0, sizeof h);
			const size_t cnt = r < G ? gstart[r + 1] - gstart[r] : n;
			for (size_t a = 0; a < cnt; a++) {
				const size_t i = r < G ? gorder[gstart[r] + a] : a;
				u64 es = 0;
				const SelMember e = sel_member(counts[i], k, K, &es);
				if (!e.n) continue;
				mem.push_back(e);
				h.sequences++;
				h.x += e.x; h.n += e.n; h.exp_r += counts[i].exp_r[k]; h.exp_s += es;
			}
			members += h.sequences;
			if (!h.sequences) mem.push_back({0u, 0u, 0.0});      // the prior alone
			mstart[r * K + k + 1] = mem.size();
		}

	// the launches: whole rows in batches of at most `cap` cells (a row of m leaves holds m + m / 2 at its first level, fewer later); a
	// row that does not fit goes alone, in blocks of P leaves (a power of two) whose roots meet on a stack as a binary counter's digits do
	ConvPlan pl;
	u32 levels = 0;
	std::vector<std::pair<const SelMember*, u32>> runs;
	std::vector<u32> outs;
	std::vector<ConvEntry> roots;
	u64 held = 0;
	auto flush = [&]() {
		if (runs.empty()) return;
		pl.reduce(runs, roots);
		pl.finish(roots, outs);
		runs.clear(); outs.clear();
		held = 0;
	};
	for (size_t q = 0; q < NR; q++) {
		const u32 m = (u32) (mstart[q + 1] - mstart[q]);
		const SelMember* lv = mem.data() + mstart[q];
		const u32 depth = conv_log2_up(m);
		levels = std::max(levels, depth);
		const u64 need = (u64) m + m / 2;
		if (need <= cap) {
			if (held + need > cap) flush();
			runs.push_back({lv, m});
			outs.push_back((u32) q);
			held += need;
			continue;
		}
		flush();
		u32 P = 1;
		while ((u64) 2 * P + P + depth + 2 <= cap) P *= 2;       // (the stack holds at most depth + 1 roots, and a combination's output)
		std::vector<ConvEntry> stack;
		for (u32 at = 0; at < m; at += P) {
			const u32 len = std::min(P, m - at);
			std::vector<std::pair<const SelMember*, u32>> one(1, {lv + at, len});
			pl.reduce(one, roots);
			stack.push_back(roots[0]);
			while (len == P && stack.size() >= 2 && stack[stack.size() - 2].w == stack.back().w) {
				const ConvEntry rr = stack.back(); stack.pop_back();
				const ConvEntry ll = stack.back(); stack.pop_back();
				stack.push_back(pl.single(ll, rr));
			}
		}
		while (stack.size() >= 2) {
			const ConvEntry rr = stack.back(); stack.pop_back();
			const ConvEntry ll = stack.back(); stack.pop_back();
			stack.push_back(pl.single(ll, rr));
		}
		pl.finish(stack, std::vector<u32>(1, (u32) q));
	}
	flush();

	HIP_TRY(hipSetDevice(c->device));
	hipStream_t st = c->stream;
	vdjx_work wk(c);
	double *d_cells, *d_pdf = nullptr;
	SelMember* d_lm;
	u32* d_lc;
	ConvJob* d_jobs;
	ConvFin* d_fins;
	vdjx_sel_stat *d_head, *d_stat;
	HIP_TRY(wk.alloc(&d_cells, (size_t) pl.ncell * SEL_T));
	HIP_TRY(wk.alloc(&d_lm, pl.leaf_m.size()));
	HIP_TRY(wk.alloc(&d_lc, pl.leaf_cell.size()));
	HIP_TRY(wk.alloc(&d_jobs, pl.jobs.size()));
	HIP_TRY(wk.alloc(&d_fins, pl.fins.size()));
	HIP_TRY(wk.alloc(&d_head, NR));
	HIP_TRY(wk.alloc(&d_stat, NR));
	if (out_pdf) HIP_TRY(wk.alloc(&d_pdf, NR * SEL_T));
	HIP_TRY(hipMemcpyAsync(d_lm, pl.leaf_m.data(), pl.leaf_m.size() * sizeof(SelMember), hipMemcpyHostToDevice, st));
	HIP_TRY(hipMemcpyAsync(d_lc, pl.leaf_cell.data(), pl.leaf_cell.size() * sizeof(u32), hipMemcpyHostToDevice, st));
	if (!pl.jobs.empty()) HIP_TRY(hipMemcpyAsync(d_jobs, pl.jobs.data(), pl.jobs.size() * sizeof(ConvJob), hipMemcpyHostToDevice, st));
	HIP_TRY(hipMemcpyAsync(d_fins, pl.fins.data(), pl.fins.size() * sizeof(ConvFin), hipMemcpyHostToDevice, st));
	HIP_TRY(hipMemcpyAsync(d_head, head.data(), NR * sizeof(vdjx_sel_stat), hipMemcpyHostToDevice, st));
	const u32 piece = 1u << 20;                          // workgroups of one launch
	for (const ConvOp& op : pl.ops) {
		if (op.kind == 0) {
			vdjx_prof_scope ps(c, "k_conv_leaf");
			hipLaunchKernelGGL(k_conv_leaf, dim3(op.count), dim3(256), 0, st, (const SelMember*) d_lm + op.start, (const u32*) d_lc + op.start, d_cells);
		} else if (op.kind == 1) {
			for (u32 a = 0; a < op.count; a += piece / CV_TILES) {
				vdjx_prof_scope ps(c, "k_conv_combine");
				hipLaunchKernelGGL(k_conv_combine, dim3(std::min(piece / CV_TILES, op.count - a) * CV_TILES), dim3(256), 0, st, d_cells,
				                   (const ConvJob*) d_jobs + op.start + a);
			}
		} else {
			vdjx_prof_scope ps(c, "k_conv_finish");
			hipLaunchKernelGGL(k_conv_finish, dim3(op.count), dim3(256), 0, st, (const double*) d_cells, (const ConvFin*) d_fins + op.start,
			                   (const vdjx_sel_stat*) d_head, d_stat, d_pdf);
		}
	}
	HIP_TRY(hipMemcpyAsync(out_stat, d_stat, NR * sizeof(vdjx_sel_stat), hipMemcpyDeviceToHost, st));
	if (out_pdf) HIP_TRY(hipMemcpyAsync(out_pdf, d_pdf, NR * SEL_T * sizeof(double), hipMemcpyDeviceToHost, st));
	HIP_TRY(hipStreamSynchronize(st));
	HIP_TRY(hipGetLastError());
	vdjx_prof_collect(c, false);
	if (info) {
		info->members = members;
		info->leaves = pl.leaf_m.size();
		info->combines = pl.jobs.size();
		info->groups = G;
		info->regions = K;
		info->rows = (u32) NR;
		info->levels = levels;
		info->batches = pl.batches;
	}
	c->stats["selconv_combines"] = pl.jobs.size();
	c->stats["selconv_batches"] = pl.batches;
	c->stats["selconv_us"] = (u64) std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
	return VDJX_OK;
}

// ---- the comparison of two densities: plain host code, no device ---------------------------------------------------------------------------
extern "C" int vdjx_selection_compare(const double* pdf, size_t rows, const uint32_t* pair, size_t P, const uint8_t* skip, vdjx_sel_test* out) {
	if (P == 0) return VDJX_OK;
	if (!pdf || !pair || !out) { vdjx_set_error("vdjx_selection_compare: NULL argument"); return VDJX_EINVAL; }
	for (size_t p = 0; p < P; p++)
		if (pair[2 * p] >= rows || pair[2 * p + 1] >= rows) { vdjx_set_error("vdjx_selection_compare: pair %zu: rows %u and %u of %zu", p, pair[2 * p], pair[2 * p + 1], rows); return VDJX_EINVAL; }
	std::vector<size_t> live;
	for (size_t p = 0; p < P; p++) {
		out[p].p_greater = out[p].pvalue = out[p].fdr = 0.0;
		if (skip && skip[p]) continue;
		const double* a = pdf + (size_t) pair[2 * p] * SEL_T;
		const double* b = pdf + (size_t) pair[2 * p + 1] * SEL_T;
		double sa = 0.0, sb = 0.0;
		for (int t = 0; t < SEL_T; t++) { sa += a[t]; sb += b[t]; }
		double below = 0.0, pg = 0.0;                    // t ascending: the mass of b below t
		for (int t = 0; t < SEL_T; t++) {
			const double bt = b[t] / sb;
			pg += a[t] / sa * (below + 0.5 * bt);
			below += bt;
		}
		pg = std::min(pg, 1.0);                           // (a probability: the sums round)
		out[p].p_greater = pg;
		out[p].pvalue = std::min(1.0, std::max(0.0, 2.0 * std::min(pg, 1.0 - pg)));
		live.push_back(p);
	}
	// Benjamini-Hochberg over the rows that take part: ascending by pvalue, ties by row order
	std::stable_sort(live.begin(), live.end(), [&](size_t x, size_t y) { return out[x].pvalue < out[y].pvalue; });
	double run = 1.0;
	for (size_t j = live.size(); j >= 1; j--) {
		run = std::min(run, out[live[j - 1]].pvalue * (double) live.size() / (double) j);
		out[live[j - 1]].fdr = std::min(1.0, run);
	}
	return VDJX_OK;
}
