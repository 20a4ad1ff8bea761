"""A repertoire with families: the input of the e2e_families golden (tests/golden/make_golden_families.py) and of tests/test_gpu_tables.py.

Every clone has a V and a J germline SEQUENCE of its own (as make_repertoire(private_v=True, private_j=True) makes them), so a tiled clone is
one contig, whatever its neighbours are.  The assembly never reads ig_vdj.fa, so the NAMES written there are free: families are made by
naming the private sequences as alleles of one gene, as genes that normalise to one gene (IGHV1-69 / IGHV1-69D, IGHV3-30 / IGHV3-30-5,
IGKV1-39 / IGKV1D-39), or by writing one sequence under two names (a tied call).  The CDR3 cores are designed: a lineage's members differ
from their founder by stated substitutions, one of them in the middle of the core (no 35-mer is shared by two clones).

    build()             -> Families: the synth.Repertoire, the FASTA records, the expected gene strings and lineages, all from SEED
    write_ref_dir(f, d)    the --ref-dir of the case (v_region.fa, v_index, j_index, ig_vdj.fa with the V, J and D records)
    write_cfa(f, path)     the constant-region FASTA of --cfa
    pool(f)                synth.tile_reads of every clone (generated when needed, never stored)
"""
from __future__ import annotations

import functools
import os
from dataclasses import dataclass, field

import numpy as np

from vdjer_amd import synth

SEED = 20261018
TAG = "e2e_families"
N_SINGLE = 70                                            # clones of a (vgene, jgene) pair of their own
COPIES, STEP = 3, 1                                      # synth.tile_reads' arguments
FLAGS = []                                               # the reference's defaults (--k 35 --mf 3 --mq 90 --mrs 30)
WINDOW_SPAN, J_EXTENSION = 360, 87                       # the reference's contig: 360 bases, 87 of them past the junction
J_RECORD = 48                                            # bases of a J + constant tail written to ig_vdj.fa (a germline J is about that long)
# The clone without a J record must get no J call by chance either: a contig of 486 random bases reaches min_j_score = 20 (ten matches in
# a row) against some ninety J records more often than not, so that clone's sequences come from the first stream (seed, k) for which the
# integer model finds no J record scoring 20 or more on its window -- found once (make_golden_families.py asserts it), written down here.
LONE_STREAM = 2
CONST_NAMES = ["IGHM*01", "IGHG1*01", "IGHG2*01", "IGHG4*01", "IGHG3*01", "IGHA1*01", "IGHE*01", "IGHD*01"]


@dataclass
class Clone:
    v_names: list                                        # the names the clone's V sequence is written under (more than one: a tied call)
    j_names: list                                        # [] : the J is left out of the FASTA
    core: str
    vgene: str                                           # what --clones / --lineages print for the V call, written down by hand
    jgene: str                                           # "" without a J record
    lineage: str = ""                                    # the designed lineage at 0.15 ("" : alone)
    part: str = ""                                       # the designed lineage at 0.05, where it differs
    d_name: str = ""                                     # the D record cut from this core

    @property
    def junction(self):
        return "TGT" + self.core + "TGG"


@dataclass
class Families:
    rep: synth.Repertoire
    clones: list
    germline: list = field(default_factory=list)        # (header, sequence as written, wrap) of ig_vdj.fa, V and J and D records interleaved
    constant: list = field(default_factory=list)        # (name, sequence) of the constant FASTA
    d_cuts: dict = field(default_factory=dict)          # D name -> sequence

    def by_junction(self):
        return {c.junction: k for k, c in enumerate(self.clones)}


def _core_ok(core):
    """no Cys codon in the first nine bases and no Trp codon in the last ten, in any frame: the window finder searches 16 bases past either
    anchor, a second candidate in the designed frame gives the same window under a shorter junction, and which of the two it reports is
    decided by the iteration order of a hash set"""
    head, tail = ("TGT" + core)[1:12], (core + "TGG")[-13:-1]
    return "TGT" not in head and "TGC" not in head and "TGG" not in tail


def _core(rng, codons):
    while True:
        core = synth._rand_codons(rng, codons)
        if _core_ok(core):
            return core


def windows(fam):
    """the contig the reference reports for every clone: WINDOW_SPAN bases that end J_EXTENSION bases past the junction"""
    out = []
    for t, c in zip(fam.rep.clones, fam.clones):
        start = 297 - (WINDOW_SPAN - (len(c.junction) + J_EXTENSION))
        out.append(t[start:start + WINDOW_SPAN])
    return out


def _subst(core, positions, rng):
    """core with the bases at `positions` changed, never into a stop codon (the frame is the core's own)"""
    s = list(core)
    for q in positions:
        for nb in rng.permutation(list("ACGT")).tolist():
            cod = s[q - q % 3:q - q % 3 + 3]
            cod[q % 3] = nb
            if nb != s[q] and "".join(cod) not in synth._STOPS:
                s[q] = nb
                break
        else:
            raise AssertionError("no substitution without a stop")
    out = "".join(s)
    assert sum(a != b for a, b in zip(out, core)) == len(positions)
    return out


def _v_germ(rng):
    """99 random codons and the Cys codon, as synth.make_repertoire makes a V -- but no other TGT / TGC, in any frame, from the V anchor
    (277) on: the reference's window finder takes every Cys codon after the anchor as a candidate and keeps the longest window"""
    while True:
        v = synth._rand_codons(rng, 99) + "TGT"
        if "TGT" not in v[270:299] and "TGC" not in v[270:299]:
            return v


def _j_germ(rng):
    """the Trp codon and 119 random codons -- but no other TGG, in any frame, in the 24 bases the window finder searches for the J residue"""
    while True:
        j = "TGG" + synth._rand_codons(rng, 119)
        if "TGG" not in j[1:27]:
            return j


@functools.lru_cache(maxsize=None)
def build(seed: int = SEED, lone_stream: int = LONE_STREAM) -> Families:
    rng = np.random.default_rng(seed)
    cl = []
    # ---- clones of a gene pair of their own: N_SINGLE distinct V genes over six J genes
    for i in range(N_SINGLE):
        cl.append(Clone([f"IGHV{1 + i % 7}-{100 + i}*01"], [f"IGHJ{1 + i % 6}*{10 + i:02d}"], _core(rng, 9 + i % 12), f"IGHV{1 + i % 7}-{100 + i}", f"IGHJ{1 + i % 6}"))

    def family(tag, v_names, vgene, j_gene, codons, steps, part=None):
        """a lineage: the founder and, per entry of `steps`, the founder with that many substitutions: one beside the middle of the core
        (no 35-mer is shared with the founder or a sibling), the others anywhere else, no position used by two members -- so two members
        are as far apart as their steps added up"""
        f = _core(rng, codons)
        L = len(f)
        free = [q for q in rng.permutation(L).tolist() if not L // 2 - 1 <= q <= L // 2 + 2 and 9 <= q < L - 10]
        for k, (vn, d) in enumerate(zip(v_names, [0] + steps)):
            pos = [L // 2 - 2 + k] + [free.pop() for _ in range(d - 1)] if d else []
            names = vn if isinstance(vn, list) else [vn]
            cl.append(Clone(names, [f"{j_gene}*{100 + len(cl)}"], _subst(f, pos, rng), vgene, j_gene, tag, (part or {}).get(k, "")))

    # alleles of one gene, three members: d = 1 and 3 from the founder (0.05 of 48 bases is two substitutions: the third member leaves)
    family("alleles", ["IGHV1-2*01", "IGHV1-2*02", "IGHV1-2*04"], "IGHV1-2", "IGHJ4", 14, [1, 3], part={2: "alleles_b"})
    # IGHV3-30 / IGHV3-30-5 normalise to one gene.  L = 48: linked up to d = 7 at 0.15, up to d = 2 at 0.05.  The second member is two
    # substitutions from the founder, the third six: it leaves the lineage at 0.05
    family("splits", ["IGHV3-30*02", "IGHV3-30-5*01", "IGHV3-30*04"], "IGHV3-30", "IGHJ6", 14, [2, 6], part={2: "splits_b"})
    # IGKV1-39 / IGKV1D-39 (the D inside the name is dropped), four members
    family("d_inside", ["IGKV1-39*01", "IGKV1D-39*01", "IGKV1-39*02", "IGKV1D-39*02"], "IGKV1-39", "IGHJ5", 16, [1, 2, 4], part={3: "d_inside_b"})
    # two lineages in one bucket (one gene pair, one junction length), and the same gene pair at another length
    family("bucket_a", ["IGHV4-4*01", "IGHV4-4*02", "IGHV4-4*07"], "IGHV4-4", "IGHJ3", 15, [1, 2])
    family("bucket_b", ["IGHV4-4*08", "IGHV4-4*09"], "IGHV4-4", "IGHJ3", 15, [3], part={1: "bucket_b_b"})
    family("other_length", ["IGHV4-4*10", "IGHV4-4*11"], "IGHV4-4", "IGHJ3", 17, [2])
    # one sequence under two names that normalise to one gene (sl_add merges them), in a lineage with a third allele
    family("tied_merged", [["IGHV1-69*01", "IGHV1-69D*01"], "IGHV1-69*02"], "IGHV1-69", "IGHJ2", 13, [1])
    # two members whose junctions translate alike (GCA / GCC in the middle codon): one cluster key of --clones found twice
    f = _core(rng, 14)
    for name, cod in (("IGHV5-51*01", "GCA"), ("IGHV5-51*03", "GCC")):
        cl.append(Clone([name], [f"IGHJ4*{100 + len(cl)}"], f[:21] + cod + f[24:], "IGHV5-51", "IGHJ4", "synonymous"))
    # one sequence under two genes: a comma-joined vgene; its J under two genes as well
    cl.append(Clone(["IGHV4-34*01", "IGHV4-59*01"], ["IGHJ1*01", "IGHJ2P*01"], _core(rng, 12), "IGHV4-34,IGHV4-59", "IGHJ1,IGHJ2P"))
    # a clone whose J is not in the FASTA: a V call and no J call
    cl.append(Clone(["IGHV7-81*01"], [], _core(rng, 11), "IGHV7-81", ""))

    n = len(cl)
    v_germ = [_v_germ(rng) for _ in range(n)]
    j_germ = [_j_germ(rng) for _ in range(n)]
    lone = np.random.default_rng([seed, lone_stream])    # the clone without a J record: a stream of its own (see LONE_STREAM)
    cl[-1].core, v_germ[-1], j_germ[-1] = _core(lone, 11), _v_germ(lone), _j_germ(lone)
    clones = [v_germ[k] + c.core + j_germ[k] for k, c in enumerate(cl)]
    w = np.full(n, 1.0 / n)
    rep = synth.Repertoire(v_germ, j_germ, clones, list(range(n)), list(range(n)), w, seed)
    rep.v_anchors = [v[277:293] for v in v_germ]
    rep.j_anchors = [j[8:24] for j in j_germ]
    assert len(set(rep.v_anchors)) == n and len(set(rep.j_anchors)) == n and len({c.junction for c in cl}) == n
    fam = Families(rep, cl)

    # ---- class-D records: cuts from the middle of six cores (tests/test_gpu_dcall.py::d_records), a duplicate of the first (a tied d_call)
    # and five random decoys
    d_recs = []
    for i in range(6):
        core = cl[i * 11].core
        k = min(14 + i, len(core))
        o = (len(core) - k) // 2
        name = f"IGHD{i + 1}-{i + 1}*01"
        cl[i * 11].d_name = name
        d_recs.append((name, core[o:o + k]))
    d_recs.append(("IGHD1-26*01", d_recs[0][1]))
    for k in range(5):
        d_recs.append((f"IGHD7-{30 + k}*01" if k % 2 else f"D{k}", "".join("ACGT"[x] for x in rng.integers(0, 4, int(rng.integers(11, 38))))))
    fam.d_cuts = dict(d_recs)

    # ---- ig_vdj.fa: per clone its V record(s) and its J record(s), a D record after every eighth clone; IMGT-shaped headers now and then,
    # one V record in lower case over wrapped lines
    recs = []
    for k, c in enumerate(cl):
        for a, name in enumerate(c.v_names):
            head = f"M{k:05d}|{name}|Homo sapiens|F|V-REGION" if (k + a) % 3 == 0 else f"{name} synthetic" if k % 3 == 1 else name
            recs.append((head, v_germ[k].lower() if k == 5 else v_germ[k], 60 if k in (5, 9) else 0))
        for a, name in enumerate(c.j_names):
            head = f"J{k:05d}|{name}|Homo sapiens" if (k + a) % 4 == 0 else name
            recs.append((head, j_germ[k][:J_RECORD], 30 if k == 7 else 0))
        if k % 8 == 7 and d_recs:
            name, s = d_recs.pop(0)
            recs.append((f"X{k}|{name}|synthetic" if k % 16 == 7 else f"{name} synthetic", s, 0))
    recs += [(name, s, 0) for name, s in d_recs]
    fam.germline = recs

    # ---- the constant FASTA (tests/test_gpu_isotype.py::constant_records): the J + tail segments of six clones downstream of the J anchor;
    # IGHG2 and IGHG4 are point-mutated copies of IGHG1, IGHG2's mutation past every tail (a tie), IGHG4's inside them
    def point(s, q):
        return s[:q] + ("A" if s[q] != "A" else "C") + s[q + 1:]

    src = [N_SINGLE, 1, N_SINGLE + 3, 2, N_SINGLE + 6, N_SINGLE + 10]      # lineage founders and single clones
    seg = [j_germ[k][24:] for k in src]
    fam.constant = list(zip(CONST_NAMES, [seg[0], seg[1], point(seg[1], 200), point(seg[1], 40), seg[2], seg[3], seg[4], seg[5]]))
    return fam


def records(fam):
    """[(FASTA header, cleaned sequence)] of ig_vdj.fa, as api.Context.germline_load / dsegment_load take them"""
    return [(h, s.upper()) for h, s, _ in fam.germline]


def _write_fasta(path, recs):
    with open(path, "w") as f:
        for head, s, wrap in recs:
            f.write(">" + head + "\n")
            if wrap:
                f.write("".join(s[q:q + wrap] + "\n" for q in range(0, len(s), wrap)))
            else:
                f.write(s + "\n")


def write_ref_dir(fam, path):
    synth.write_ref_dir(fam.rep, path)
    _write_fasta(os.path.join(path, "ig_vdj.fa"), fam.germline)
    return path


def write_cfa(fam, path):
    _write_fasta(path, [(f"{name} constant" if k % 2 else f"X{k}|{name}|synthetic", s, 70 if k == 2 else 0) for k, (name, s) in enumerate(fam.constant)])


def pool(fam):
    return synth.tile_reads(fam.rep, list(range(len(fam.clones))), copies=COPIES, step=STEP)


def argv():
    return ["--in", "reads.txt", "--chain", "IGH", "--ref-dir", "ref", "--ins", "175", "--t", "1"] + FLAGS


def golden_contigs(text):
    """(ids, contigs) of vdj_contigs.fa's text"""
    fa = text.splitlines()
    return [fa[i][1:] for i in range(0, len(fa), 2)], [fa[i + 1] for i in range(0, len(fa), 2)]


def hamming(a, b):
    return sum(x != y for x, y in zip(a, b))


def designed(fam, ids, contigs):
    """What the tables must show for these contigs BY DESIGN (gene strings written down in build(), junctions from the contig ids): per
    contig the clone it is a verbatim window of (or None), and the conditions of the golden as a dict of counts.  No aligner is involved."""
    at = fam.by_junction()
    who = []
    for cid, s in zip(ids, contigs):
        k = at.get(cid.split("_", 2)[2])
        who.append(k if k is not None and s in fam.rep.clones[k] else None)
    elig = [c for c, k in enumerate(who) if k is not None and fam.clones[k].j_names]
    groups, lengths = {}, {}
    for c in elig:
        x = fam.clones[who[c]]
        groups.setdefault((x.vgene, x.jgene), []).append(c)
    lin15, lin05 = {}, {}
    for c in elig:
        x = fam.clones[who[c]]
        lin15.setdefault(x.lineage or f"alone_{who[c]}", []).append(c)
        lin05.setdefault(x.part or x.lineage or f"alone_{who[c]}", []).append(c)
    buckets = {}
    for name, members in lin15.items():
        x = fam.clones[who[members[0]]]
        buckets.setdefault((x.vgene, x.jgene, len(x.junction)), []).append(name)
    for (vg, jg, L) in buckets:
        lengths.setdefault((vg, jg), set()).add(L)
    allele_spread = [name for name, members in lin15.items()
                     if len(members) >= 2 and len({fam.clones[who[c]].v_names[0] for c in members}) >= 2 and len({fam.clones[who[c]].v_names[0].split("*")[0] for c in members}) == 1]
    return who, dict(contigs=len(ids), verbatim=sum(k is not None for k in who), eligible=len(elig), groups=len(groups),
                     lineages_of_3=sum(len(m) >= 3 for m in lin15.values()), lineages=len(lin15), lineages_at_005=len(lin05),
                     buckets_of_2_lineages=sum(len(v) >= 2 for v in buckets.values()), groups_of_2_lengths=sum(len(v) >= 2 for v in lengths.values()),
                     allele_lineages=len(allele_spread), ineligible=len(ids) - len(elig),
                     tied_vgenes=sum("," in fam.clones[k].vgene for k in who if k is not None))


def check_conditions(cond):
    """the conditions that make tests/test_gpu_tables.py non-vacuous"""
    assert cond["groups"] >= 65, cond                    # the 65th distinct key: the key tables of clones_table / lineage_run grow
    assert cond["lineages_of_3"] >= 3, cond
    assert cond["buckets_of_2_lineages"] >= 1 and cond["groups_of_2_lengths"] >= 1, cond
    assert cond["allele_lineages"] >= 1 and cond["lineages_at_005"] > cond["lineages"], cond
    assert cond["ineligible"] >= 1 and cond["tied_vgenes"] >= 1, cond


def check_design(fam):
    """the design itself: the members of a lineage hang together at 0.15 and the families lie apart, the designed split happens at 0.05,
    no two clones share a 35-mer"""
    by = {}
    for c in fam.clones:
        if c.j_names:
            by.setdefault((c.vgene, c.jgene, len(c.junction)), []).append(c)
    for members in by.values():
        for a in members:
            for b in members:
                if a is b:
                    continue
                d, L = hamming(a.junction, b.junction), len(a.junction)
                same15, same05 = bool(a.lineage) and a.lineage == b.lineage, bool(a.lineage) and (a.part or a.lineage) == (b.part or b.lineage)
                if not same15:
                    assert d * 10000 > 1500 * L, (a, b)
                if not same05:
                    assert d * 10000 > 500 * L, (a, b)
            if a.lineage:                                # linked to the founder-side member it was made from, directly
                mates = [b for b in members if b is not a and b.lineage == a.lineage]
                assert min(hamming(a.junction, b.junction) for b in mates) * 10000 <= 1500 * len(a.junction), a
                near = [b for b in mates if (b.part or b.lineage) == (a.part or a.lineage)]
                assert not near or min(hamming(a.junction, b.junction) for b in near) * 10000 <= 500 * len(a.junction), a
    assert all(_core_ok(c.core) for c in fam.clones)
    seen = {}
    for k, t in enumerate(fam.rep.clones):
        for q in range(len(t) - 34):
            assert seen.setdefault(t[q:q + 35], k) == k, (k, q)
