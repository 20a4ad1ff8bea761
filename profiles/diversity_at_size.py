"""vdjx_diversity at size, B = 200 replicates: one JSON line per leg with the info, the best-of-three host time of the call
after a warm-up, each kernel's own time (HIP events, one more call) and the draws per second by the draw kernel's time and by the call's.
   python profiles/diversity_at_size.py [out.json]
   python profiles/diversity_at_size.py bounds [out.json]
     lineages_2172      2,172 Zipf-weighted lineages (the size of the profiles/annot_at_size.py input) at N = 100,000: the LDS histogram;
                        again with VDJX_DIV_LDS_CLONES=0 (every draw a global atomicAdd), and the numpy path of tests/diversity_model.py
                        (counts of all replicates; the Hill numbers of one, scaled) on the same input
     clones_1m          one call of 2^20 - 1 Zipf-weighted clones at N = 10^7: the global path, one batch of 200 x (2^20 - 1) counters
     quant_e2e_mixed    the quant step (vdjx_quant) on the e2e_mixed golden, to compare against
`bounds`: what bounds each kernel -- the draw kernel at ten times the draws (its fixed cost: zeroing and flushing the histograms), with
all weight on one clone (every LDS atomic of a wave on one counter), with equal weights, and at 1,024 clones (the whole search in LDS);
the Hill kernel on the second input at 41 orders, at the orders 0, 1, 2 (one pow per value) and at order 0 alone (none).
With a file name the legs are written there as well, as profiles/diversity_at_size.json holds them."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B = 200
KERNELS = ["k_div_draw", "k_div_hill", "k_div_fin"]


def zipf(rng, C, s=1.1):
    """integer Zipf weights in random order, none of them 0"""
    w = np.maximum(1, 1e9 / np.arange(1, C + 1, dtype=np.float64) ** s).astype(np.uint64)
    return w[rng.permutation(C)]


def leg(ctx, name, weight, N, env=None):
    for k in ("VDJX_DIV_CELLS", "VDJX_DIV_LDS_CLONES"):
        os.environ.pop(k, None)
    os.environ.update(env or {})
    ctx.diversity(weight[:64], 1000, replicates=2)                      # (warm-up: code objects)
    ctx.diversity(weight, N, replicates=B)                              # (... and the workspace)
    best = None
    for _ in range(3):
        t0 = time.perf_counter()
        res = ctx.diversity(weight, N, replicates=B)
        wall = time.perf_counter() - t0
        cur = (ctx.stat("diversity_us"), wall)
        best = cur if best is None or cur[0] < best[0] else best
    ctx.profile(True)
    ctx.profile_reset()
    ctx.diversity(weight, N, replicates=B)
    prof = ctx.profile_get()
    ctx.profile(False)
    ms = {k: prof.get(k, (0.0, 0))[0] for k in KERNELS}
    drawn = int(round(float(res["mean"][0])))
    out = dict(leg=name, env=env or {}, **res["info"], orders=int(res["d"].shape[1]), call_ms=round(best[0] / 1e3, 3), wall_ms=round(best[1] * 1e3, 3),
               kernel_ms={k: round(v, 4) for k, v in ms.items()}, dispatches={k: v[1] for k, v in prof.items()},
               draws=B * N, draws_per_s_kernel=round(B * N / (ms["k_div_draw"] / 1e3)), draws_per_s_call=round(B * N / (best[0] / 1e6)),
               mean_clones_drawn=drawn, pow_calls=B * drawn * (int(res["d"].shape[1]) - 2),
               pows_per_s_kernel=round(B * drawn * (int(res["d"].shape[1]) - 2) / (ms["k_div_hill"] / 1e3)),
               richness=round(float(res["mean"][0]), 2), shannon=round(float(res["mean"][10]), 4), simpson=round(float(res["mean"][20]), 4),
               simpson_sd=round(float(res["sd"][20]), 4), observed_richness=float(res["observed"][0]))
    print(json.dumps(out), flush=True)
    return out


def kernel_ms(ctx, weight, N, q=None, env=None):
    for k in ("VDJX_DIV_CELLS", "VDJX_DIV_LDS_CLONES"):
        os.environ.pop(k, None)
    os.environ.update(env or {})
    ctx.diversity(weight, N, q, replicates=B)                           # (warm-up)
    best = None
    for _ in range(3):
        ctx.profile(True)
        ctx.profile_reset()
        res = ctx.diversity(weight, N, q, replicates=B)
        prof = ctx.profile_get()
        ctx.profile(False)
        ms = {k: round(prof.get(k, (0.0, 0))[0], 4) for k in KERNELS}
        best = ms if best is None or ms["k_div_draw"] + ms["k_div_hill"] < best["k_div_draw"] + best["k_div_hill"] else best
    return best, int(round(float(res["mean"][0]))) if (res["d"].shape[1] > 1 or q is None or q[0] == 0.0) else None


def bounds():
    from vdjer_amd import api
    ctx = api.Context(0)
    rng = np.random.default_rng(2172)
    small = zipf(rng, 2172)
    hot = np.ones(2172, np.uint64)
    hot[1000] = 10 ** 12
    legs = []

    def draw(name, w, N, env=None):
        ms, drawn = kernel_ms(ctx, w, N, [0.0], env)
        legs.append(dict(leg=name, clones=len(w), depth=N, draw_ms=ms["k_div_draw"], ns_per_1000_draws=round(ms["k_div_draw"] * 1e6 / (B * N) * 1e3, 3), clones_drawn=drawn))
        print(json.dumps(legs[-1]), flush=True)

    draw("zipf_2172_1e5", small, 10 ** 5)
    draw("zipf_2172_1e6", small, 10 ** 6)
    draw("one_hot_clone_2172_1e6", hot, 10 ** 6)
    draw("equal_2172_1e6", np.ones(2172, np.uint64), 10 ** 6)
    draw("zipf_1024_1e6", zipf(rng, 1024), 10 ** 6)
    draw("zipf_16384_1e6", zipf(rng, 16384), 10 ** 6)
    draw("zipf_2172_1e6_global", small, 10 ** 6, dict(VDJX_DIV_LDS_CLONES="0"))
    draw("one_hot_clone_2172_1e6_global", hot, 10 ** 6, dict(VDJX_DIV_LDS_CLONES="0"))
    big = zipf(rng, (1 << 20) - 1)
    for name, q in (("hill_1m_41_orders", None), ("hill_1m_orders_0_1_2", [0.0, 1.0, 2.0]), ("hill_1m_order_0", [0.0])):
        ms, drawn = kernel_ms(ctx, big, 10 ** 7, q)
        nq = 41 if q is None else len(q)
        legs.append(dict(leg=name, clones=len(big), depth=10 ** 7, orders=nq, hill_ms=ms["k_div_hill"], draw_ms=ms["k_div_draw"], clones_drawn=drawn,
                         pow_calls=B * drawn * max(0, nq - 2)))
        print(json.dumps(legs[-1]), flush=True)
    ctx.close()
    return legs


def numpy_leg(weight, N):
    from tests import diversity_model as M
    w = [int(x) for x in weight]
    t0 = time.perf_counter()
    cs = [M.counts(w, N, 1, r) for r in range(1, B + 1)]
    t_counts = time.perf_counter() - t0
    t0 = time.perf_counter()
    [M.hill(cs[0], N, q) for q in M.orders()]
    t_hill = (time.perf_counter() - t0) * B
    out = dict(leg="lineages_2172_numpy_model", clones=len(w), depth=N, replicates=B, counts_ms=round(t_counts * 1e3, 1),
               hill_ms_one_replicate_times_B=round(t_hill * 1e3, 1), draws_per_s=round(B * N / t_counts))
    print(json.dumps(out), flush=True)
    return out


def quant_leg(ctx):
    from tests import golden_util as G
    c = G.Case("e2e_mixed")
    fa = G.text("e2e_mixed.contigs.fa.gz").splitlines()
    seqs = [fa[i + 1] for i in range(0, len(fa), 2)]
    p = ctx.pool_load(c.pool.primary, c.pool.secondary, c.pool.rl)
    ctx.read_index_build(p, c.pool.pair_id, c.pool.read_num, c.pool.is_rc, c.pool.reg_rank, c.pool.n_pairs)
    packed = ctx.pack_strings(seqs)
    ctx.quant(packed)                                                   # (warm-up: code objects, workspace)
    runs = []
    for _ in range(3):
        t0 = time.perf_counter()
        _, info = ctx.quant(packed)
        runs.append(time.perf_counter() - t0)
    p.free()
    out = dict(leg="quant_e2e_mixed", contigs=len(seqs), pairs=info["pairs"], iterations=info["iterations"], quant_ms=round(min(runs) * 1e3, 3))
    print(json.dumps(out), flush=True)
    return out


def at_size():
    from vdjer_amd import api
    ctx = api.Context(0)
    rng = np.random.default_rng(2172)
    small = zipf(rng, 2172)
    legs = [leg(ctx, "lineages_2172", small, 100000), leg(ctx, "lineages_2172_global", small, 100000, dict(VDJX_DIV_LDS_CLONES="0")),
            numpy_leg(small, 100000), leg(ctx, "clones_1m", zipf(rng, (1 << 20) - 1), 10 ** 7), quant_leg(ctx)]
    ctx.close()
    return legs


if __name__ == "__main__":
    mode = "bounds" if sys.argv[1:2] == ["bounds"] else "at_size"
    legs = bounds() if mode == "bounds" else at_size()
    out = sys.argv[2:3] if mode == "bounds" else sys.argv[1:2]
    if out:
        with open(out[0], "w") as f:
            json.dump(dict(what=f"profiles/diversity_at_size.py{' bounds' if mode == 'bounds' else ''}, as printed", where="one MI355X", replicates=B, legs=legs), f, indent=1)
            f.write("\n")
