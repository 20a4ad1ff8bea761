"""vdjx_lineage_link at size: per input and linkage the best-of-five host time of the call after a warm-up, the time of
k_link_matrix and k_link_merge (HIP events, a sixth call) next to k_lin_pairs on the same input, the link info and merges per second.
   python profiles/lineage_link_at_size.py [out.json]
     at_size            the 2,172 contigs of the at_size_contigs recipe under their own V / J groups: buckets of one, no component of two --
                        what the new path costs a call that has nothing to agglomerate
     at_size_one_group  the same junctions under ONE group: a bucket per junction length
     one_component      one bucket that is one single-linkage component of 4,096 (a founder of 48 bases, 1 .. 5 substitutions a member):
                        ONE workgroup of k_link_merge, the matrix in the workspace
     small_components   20,000 components of 2 .. 8 in 200 groups: the LDS path, a workgroup each
With `cli <tag>`: profiles/lineage_at_size.py's cli leg (no --lineage-link: the new path is not entered)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests.test_gpu_annot import at_size_contigs  # noqa: E402

KERNELS = ["k_lin_pairs", "k_link_gather", "k_link_matrix", "k_link_merge"]


def leg(ctx, name, junctions, group, out):
    for link in ("single", "complete", "average"):
        call = (lambda j, g: ctx.lineage(j, g)) if link == "single" else (lambda j, g, link=link: ctx.lineage_link(j, g, link=link))
        call(junctions[:64], group[:64])        # (warm-up: code objects, workspace)
        call(junctions, group)
        calls, links = [], []
        for _ in range(5):
            t0 = time.perf_counter()
            res = call(junctions, group)
            wall = time.perf_counter() - t0
            calls.append(ctx.stat("lineage_us"))
            links.append(ctx.stat("lineage_link_us") if link != "single" else 0)
        ctx.profile(True)
        ctx.profile_reset()
        call(junctions, group)
        prof = ctx.profile_get()
        ctx.profile(False)
        merge_ms = prof.get("k_link_merge", (0.0, 0))[0]
        row = dict(leg=name, link=link, n=len(junctions), **res["info"], **res.get("link", {}), call_ms=round(min(calls) / 1e3, 3),
                   call_all_ms=[round(c / 1e3, 3) for c in calls], link_host_ms=round(min(links) / 1e3, 3), last_wall_ms=round(wall * 1e3, 3),
                   kernel_ms={k: round(prof.get(k, (0.0, 0))[0], 4) for k in KERNELS}, dispatches={k: v[1] for k, v in prof.items()})
        if link != "single" and merge_ms > 0:
            row["merges_per_s_kernel"] = float("%.4g" % (res["link"]["merges"] / (merge_ms * 1e-3)))
            row["merges_per_s_call"] = float("%.4g" % (res["link"]["merges"] / max(min(calls) * 1e-6, 1e-9)))
        print(json.dumps(row), flush=True)
        out.append(row)


def family(rng, founder, m, lo, hi):
    fam = np.repeat(founder[None, :], m, axis=0)
    for r in range(1, m):
        pos = rng.choice(fam.shape[1], size=int(rng.integers(lo, hi + 1)), replace=False)
        fam[r, pos] = (fam[r, pos] + rng.integers(1, 4, len(pos), dtype=np.uint8)) % 4
    return fam


def text_of(codes):
    return [bytes(r) for r in np.frombuffer(b"ACGT", np.uint8)[codes]]


def main(path):
    from vdjer_amd import api
    out = []
    ids, _, rep, clone = at_size_contigs()
    junctions = [i.split("_", 2)[2] for i in ids]
    seen = {}
    group = np.array([seen.setdefault((rep.clone_v[c], rep.clone_j[c]), len(seen)) for c in clone], np.uint32)
    ctx = api.Context(0)
    leg(ctx, "at_size", junctions, group, out)
    leg(ctx, "at_size_one_group", junctions, np.zeros(len(junctions), np.uint32), out)
    rng = np.random.default_rng(4096)
    one = family(rng, rng.integers(0, 4, 48, dtype=np.uint8), 4096, 1, 5)
    leg(ctx, "one_component", text_of(one[rng.permutation(4096)]), np.zeros(4096, np.uint32), out)
    fams, grp = [], []
    for f in range(20000):
        m = int(rng.integers(2, 9))
        fams.append(family(rng, rng.integers(0, 4, 48, dtype=np.uint8), m, 1, 3))
        grp += [f // 100] * m
    codes = np.concatenate(fams)
    order = rng.permutation(len(codes))
    leg(ctx, "small_components", text_of(codes[order]), np.asarray(grp, np.uint32)[order], out)
    ctx.close()
    if path:
        with open(path, "w") as fp:
            json.dump(dict(legs=out), fp, indent=1)
            fp.write("\n")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "cli":
        from profiles.lineage_at_size import cli
        cli(sys.argv[2] if len(sys.argv) > 2 else "e2e_mixed")
    else:
        main(sys.argv[1] if len(sys.argv) > 1 else None)
