#!/usr/bin/env python3
"""The e2e_families golden: what the compiled reference (oracle/_ref/vdjer_ref, --t 1) assembles from the repertoire of tests/families.py
-- some ninety tiled clones whose germline NAMES make families: alleles of one gene, genes that normalise to one gene, one sequence under two
genes, a clone without a J record.  Same rules as make_golden_chains.py: runs only where oracle/_ref/vdjer_ref is built, accepts only
complete runs that agree byte for byte (complete_run).

Writes tests/golden/e2e_families.contigs.fa.gz and the MANIFEST.json entry "e2e_families": flags, contigs, roots, pairs, the SHA-256 of the
SAM and of vdjer.dot (the SAM of a pool this size is too large to store; make_golden_midscale.py is the precedent), and the counts of the
conditions that make tests/test_gpu_tables.py non-vacuous (families.designed), asserted here before anything is written.
"""
from __future__ import annotations

import hashlib
import json
import os
import shutil
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
from tests import annot_model as A  # noqa: E402
from tests import families as F  # noqa: E402
from make_golden import REF, gz_write  # noqa: E402
from make_golden_chains import complete_run  # noqa: E402

LARGEST_FIXTURE = 1458744                                 # e2e_rl151.npz: no new fixture may be larger


def sha(text: str) -> dict:
    b = text.encode()
    return {"sha256": hashlib.sha256(b).hexdigest(), "bytes": len(b), "lines": b.count(b"\n")}


def main():
    assert os.path.exists(REF), "build the reference first: make -C oracle ref"
    fam = F.build()
    F.check_design(fam)
    wd = tempfile.mkdtemp(prefix="vdjx_golden_families_")
    F.write_ref_dir(fam, os.path.join(wd, "ref"))
    pool = F.pool(fam)
    pool.write_reads_file(os.path.join(wd, "reads.txt"))
    (fa, sam, dot), _, nroots = complete_run(wd, ["run"] + F.argv())
    ids, contigs = F.golden_contigs(fa)
    who, cond = F.designed(fam, ids, contigs)
    F.check_conditions(cond)
    assert cond["verbatim"] == cond["contigs"] == len(set(who)), cond          # one contig per clone, each a window of its clone
    # the clone without a J record gets no J call by chance either: no J record reaches min_j_score on its contig (the integer model)
    lone = [c for c, k in enumerate(who) if not fam.clones[k].j_names]
    jrecs = [s for h, s in F.records(fam) if A.parse_class(A.parse_name(h)) == "J"]
    assert lone and int(A.scores([contigs[c] for c in lone], jrecs).max()) < A.DEFAULT["min_j_score"], "the J-less clone has a chance J hit: another seed"
    gz_write(f"{F.TAG}.contigs.fa.gz", fa)
    assert os.path.getsize(os.path.join(HERE, f"{F.TAG}.contigs.fa.gz")) <= LARGEST_FIXTURE
    man = json.load(open(os.path.join(HERE, "MANIFEST.json")))
    man[F.TAG] = {"flags": F.FLAGS, "seed": F.SEED, "copies": F.COPIES, "step": F.STEP, "clones": len(fam.clones), "contigs": len(ids), "roots": nroots,
                  "pairs": int(pool.n_pairs), "sam": sha(sam), "dot": sha(dot), "conditions": cond}
    with open(os.path.join(HERE, "MANIFEST.json"), "w") as f:
        json.dump(man, f, indent=1, sort_keys=True)
    print(json.dumps(man[F.TAG], indent=1))
    shutil.rmtree(wd)


if __name__ == "__main__":
    main()
