#!/usr/bin/env python3
"""The edges_* fixtures: what the compiled reference returns on the edges the dumps of make_golden.py leave out (same rules as
make_golden.py: runs only where oracle/_ref/vdjer_ref exists; only dumps and settings are written, no program text).

  edges_<tag>.nodes.tsv.gz, edges_<tag>.survivors.tsv.gz   `vdjer_ref graph` on tests/ref_live.py's EDGE_GRAPH[tag]
  edges_map_<tag>.txt.gz                                   `vdjer_ref map` on EDGE_MAP[tag]
  edges.json   per tag the recipe (synth arguments, seeds, edits and flags: the configuration dict itself), the counts and the
               SHA-256 of the pool's primary and secondary bytes.  No pool is stored: the tests rebuild it from the recipe and
               compare the digest first, so that a change of synth is noticed and not mistaken for a parity failure.

    python tests/golden/make_golden_edges.py
"""
from __future__ import annotations

import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
from make_golden import gz_write  # noqa: E402
from tests import ref_live as R  # noqa: E402

LIMIT = 200_000                     # bytes per file


def main():
    assert R.available(), "build the reference first: make -C oracle ref"
    out = {"graph": {}, "map": {}}
    pools = {}
    for tag, c in R.EDGE_GRAPH.items():
        key = json.dumps({k: v for k, v in c.items() if k not in ("mf", "mq")}, sort_keys=True)      # (the six --mq configurations share a pool)
        if key not in pools:
            pools[key] = R.make_pool(c)
        rep, pool = pools[key]
        pre, surv, nodes, (surv_text, nodes_text) = R.graph(rep, pool, c["k"], c["mf"], c["mq"], timeout=R.timeout_of(c), keep_text=True)
        R.edge_conditions(tag, c, pre, surv, nodes)
        gz_write(f"edges_{tag}.survivors.tsv.gz", surv_text)
        gz_write(f"edges_{tag}.nodes.tsv.gz", nodes_text)
        out["graph"][tag] = {"recipe": c, "pre": pre, "survivors": len(surv), "nodes": len(nodes), "sha256": R.pool_sha(pool)}
        print(tag, pre, len(surv), len(nodes))
    for tag, c in R.EDGE_MAP.items():
        rep, pool, wins = R.make_map_case(c)
        ref, text = R.map_windows(rep, pool, wins, c["ins"], c["e0"], c["e1"], c["rs"], c["ms"], c["rf"], keep_text=True)
        gz_write(f"edges_map_{tag}.txt.gz", text)
        out["map"][tag] = {"recipe": c, "windows": len(wins), "valid": sum(w["valid"] for w in ref), "pairs": sum(w["n"] for w in ref),
                           "sha256": R.pool_sha(pool)}
        print(tag, len(wins), out["map"][tag]["valid"], out["map"][tag]["pairs"])
    with open(os.path.join(HERE, "edges.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    big = [(n, os.path.getsize(os.path.join(HERE, n))) for n in os.listdir(HERE) if n.startswith("edges") and os.path.getsize(os.path.join(HERE, n)) > LIMIT]
    assert not big, big


if __name__ == "__main__":
    main()
