"""The germline-row and mutation-count model (tests/mutation_model.py; include/vdjx.h, vdjx_mutations) on its own, without a GPU: counts
designed by hand, invariants on random hits, the condition of the `vdjer --mutations` golden run (tests/test_gpu_mutation.py plants the same
substitutions), and the Python mirror of the new ABI."""
import ctypes
import functools

import numpy as np

from tests import annot_model as A
from tests import dcall_model as D
from tests import families as F
from tests import golden_util as G
from tests import mutation_model as M
from tests.test_gpu_annot import _random_case


# ---- 1. designed counts ------------------------------------------------------------------------------------------------------------------
# a V germline of 30 codons; the designed codons sit at codon 5, 9, 13, 17 and 21, the first 15 and the last 24 bases are untouched
FILLER = "GAT CTG AAC GTC CAG ACT GGA TCC AAG CGT TTC ATC GAG CCA".split()
DESIGN = {5: ("GCA", "GCC", dict(v_s=1)),                  # silent: Ala -> Ala
          9: ("GCA", "GAA", dict(v_r=1)),                  # replacement: Ala -> Glu
          13: ("TGG", "TGA", dict(v_stop=1)),              # a mutation into a stop
          17: ("TAA", "TAC", dict(v_stop=1)),              # a germline stop: whatever it changes into
          21: ("GCA", "AAA", dict(v_r=2))}                 # two changes, each in the germline's context: ACA (Thr) and GAA (Glu)


def designed_pair():
    germ, cont = [], []
    for c in range(30):
        g, s, _ = DESIGN.get(c, (FILLER[(5 * c + c // 7) % len(FILLER)],) * 2 + (None,))
        germ.append(g)
        cont.append(s)
    return "".join(germ), "".join(cont)


def test_designed_counts():
    germ, cont = designed_pair()
    assert len(germ) == 90 and sum(a != b for a, b in zip(germ, cont)) == 6
    for c in DESIGN:
        assert 10 <= 3 * c and 3 * c + 3 <= 90 - 10
    contig = "TTTTTTT" + cont + "CCCCC"
    hits = A.annotate([contig], [germ], ["V"])
    v = hits["v"]
    assert v["gene"][0] == 0 and v["seq_start"][0] == 8 and v["seq_end"][0] == 97 and v["germ_start"][0] == 1 and v["germ_end"][0] == 90
    rows, counts, info = M.mutations([contig], hits["v"], None, hits["j"], None, [germ], [])
    want = dict(v_r=3, v_s=1, v_stop=2, v_na=0, v_codons=30, cols=90, j_mis=0, flags=M.F_V)
    assert {k: int(counts[k][0]) for k in M.COUNTS} == want
    assert rows["seq"][0] == cont and rows["germ"][0] == germ and rows["mask"][0] == germ
    assert info == dict(contigs=1, aligned=1, cols=90, v_r=3, v_s=1, v_stop=2, v_na=0, v_codons=30, truncated=0, clipped=0)
    # the limit at the first, second and third base of the double codon (contig positions 70, 71, 72; 0-based 7 + 63 ..): the codon is
    # not classifiable, its mismatches below the limit are unclassified
    for lim, na in ((7 + 63, 0), (7 + 64, 1), (7 + 65, 2), (7 + 66, 0)):
        _, cn, _ = M.mutations([contig], hits["v"], None, hits["j"], [lim], [germ], [])
        assert int(cn["v_na"][0]) == na and int(cn["v_r"][0]) == (3 if lim == 7 + 66 else 1) and int(cn["v_codons"][0]) == (22 if lim == 7 + 66 else 21), (lim, cn)
    # N or a lower-case base inside a mismatching codon: nothing of it is classified
    for ch in "Nc":
        bad = contig[:7 + 27] + ch + contig[7 + 28:]             # the first base of codon 9 (GAA against GCA)
        h2 = A.annotate([bad], [germ], ["V"])
        _, cn, _ = M.mutations([bad], h2["v"], None, h2["j"], None, [germ], [])
        assert (int(cn["v_r"][0]), int(cn["v_na"][0]), int(cn["v_codons"][0])) == (2, 2, 29), (ch, cn)


# ---- 2. invariants on random hits --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def random_case(seed):
    contigs, recs, germs, classes = _random_case(seed, 200)
    hits = A.annotate(contigs, germs, classes)
    ws, wl = D.d_window(hits["v"], hits["j"])
    gaps = [contigs[c][int(a):int(a) + int(l)] for c, (a, l) in enumerate(zip(ws, wl)) if l >= 14]
    d_germs = [gaps[0][3:-3], "ACGTTGCAAGT"]                        # (a D record cut from the first gap of 14 bases or more)
    d, _ = D.dcall(contigs, ws, wl, d_germs, dict(D.DEFAULT, min_score=8))
    return contigs, germs, hits, d, d_germs


def _printable(s):
    return "".join(ch if ch in "ACGT" else "N" for ch in s)


def test_invariants_on_random_hits():
    used = dict(v=0, j=0, d=0, indel=0)
    for seed in (1, 5):
        contigs, germs, hits, d, d_germs = random_case(seed)
        v, j = hits["v"], hits["j"]
        n = len(contigs)
        rng = np.random.default_rng(seed)
        limit = rng.integers(0, 201, n)
        off = M.layout(v, d, j)
        for lim in (None, limit):
            rows, counts, info = M.mutations(contigs, v, d, j, lim, germs, d_germs)
            for c in range(n):
                cols, flags, _ = M.columns(c, v, d, j)
                assert len(rows["seq"][c]) == len(rows["germ"][c]) == len(rows["mask"][c]) == counts["cols"][c] == int(off[c + 1] - off[c])
                if not flags & M.F_V:
                    assert counts["cols"][c] == 0 and not any(int(counts[k][c]) for k in M.COUNTS if k != "flags")
                    continue
                end = int(j["seq_end"][c]) if flags & M.F_J else int(v["seq_end"][c])
                assert rows["seq"][c].replace("-", "") == contigs[c][int(v["seq_start"][c]) - 1:end]
                nv = sum(int(r) >> 4 for r in v["runs"][c][:int(v["n_runs"][c])])
                g = germs[int(v["gene"][c])]
                assert rows["germ"][c][:nv].replace("-", "") == _printable(g[int(v["germ_start"][c]) - 1:int(v["germ_end"][c])])
                # the V mismatch columns below the limit, counted from the rows alone
                L = 200 if lim is None else int(lim[c])
                p, mism = int(v["seq_start"][c]) - 1, 0
                for a, b in zip(rows["seq"][c][:nv], rows["germ"][c][:nv]):
                    if a != "-" and b != "-" and p < L and (a != b or a not in "ACGT"):
                        mism += 1
                    p += a != "-"
                assert int(counts["v_r"][c] + counts["v_s"][c] + counts["v_stop"][c] + counts["v_na"][c]) == mism
                if lim is None:
                    assert mism == int(v["mismatches"][c])
                for k, (reg, _, _, _) in enumerate(cols):
                    assert rows["mask"][c][k] == ("N" if reg == "G" else rows["germ"][c][k])
                used["v"] += 1
                used["j"] += bool(flags & M.F_J)
                used["d"] += bool(flags & M.F_D)
                used["indel"] += "-" in rows["seq"][c][:nv] or "-" in rows["germ"][c][:nv]
            assert info["cols"] == int(off[n]) and info["contigs"] == n
    assert min(used.values()) > 0, used


# ---- 3. the condition of the CLI golden --------------------------------------------------------------------------------------------------
KINDS = ["S", "R", "stop", "RR"]
WANT = {"S": dict(v_s=1), "R": dict(v_r=1), "stop": dict(v_stop=1), "RR": dict(v_r=2)}


def _classes(germ_codon, contig_codon):
    """the class of every differing position, by the rule written in include/vdjx.h (the genetic code: annot_model.translate)"""
    out = []
    for b in range(3):
        if germ_codon[b] != contig_codon[b]:
            ch = germ_codon[:b] + contig_codon[b] + germ_codon[b + 1:]
            ga, ca = A.translate(germ_codon), A.translate(ch)
            out.append("stop" if "*" in (ga, ca) else "S" if ga == ca else "R")
    return out


def _plant_codon(v, lo, hi, kind):
    """a germline codon for the contig's codon at some codon position inside v[lo:hi) that makes the contig show `kind` -> (base offset of
    the codon, the planted codon)"""
    want = {"S": ["S"], "R": ["R"], "stop": ["stop"], "RR": ["R", "R"]}[kind]
    mid = (lo + hi) // 6
    for c in sorted(range((lo + 2) // 3, hi // 3), key=lambda c: abs(c - mid)):
        x = v[3 * c:3 * c + 3]
        for g in (a + b + d for a in "ACGT" for b in "ACGT" for d in "ACGT"):
            if _classes(g, x) == want:
                return 3 * c, g
    raise AssertionError(("no codon to plant", kind))


@functools.lru_cache(maxsize=None)
def planted_families():
    """the ig_vdj.fa records of tests/families.py with designed substitutions planted in the V records of ten clones (the assembly never
    reads the FASTA: the contigs are the golden's) -> (ids, contigs, records as written [(head, seq, wrap)], {contig index: (kind, V
    position of the planted codon)})"""
    fam = F.build()
    ids, seqs = F.golden_contigs(G.text(f"{F.TAG}.contigs.fa.gz"))
    who, _ = F.designed(fam, ids, seqs)
    recs = [list(r) for r in fam.germline]
    planted, done = {}, set()
    for c, k in enumerate(who):
        if k is None or k in done or len(fam.clones[k].v_names) != 1 or not fam.clones[k].j_names or len(planted) == 10:
            continue
        done.add(k)
        v = fam.rep.v_germ[k]
        start = fam.rep.clones[k].find(seqs[c])                      # the part of the V that the contig holds: v[start:300]
        assert 0 <= start < 200
        kind = KINDS[len(planted) % len(KINDS)]
        at, codon = _plant_codon(v, start + 10, 290, kind)
        hit = [r for r in recs if r[1].upper() == v]
        assert len(hit) == 1
        s = hit[0][1]
        hit[0][1] = s[:at] + (codon.lower() if s.islower() else codon) + s[at + 3:]
        planted[c] = (kind, at, start)
    assert len(planted) == 10
    return ids, seqs, [tuple(r) for r in recs], planted


def parsed_records(recs):
    """(names, classes, sequences, D names, D sequences) of FASTA records, by the rules of include/vdjx.h (annot_model's)"""
    names = [A.parse_name(h) for h, _, _ in recs]
    classes = [A.parse_class(x) for x in names]
    seqs = [A.clean(s) for _, s, _ in recs]
    dn = [x for x, c in zip(names, classes) if c == "D"]
    ds = [s for s, c in zip(seqs, classes) if c == "D"]
    return names, classes, seqs, dn, ds


def _v_hits(contigs, germs, own):
    """vdjx_annot_hit fields of contig k against record own[k] alone (annot_model's traceback), and a J side without a call"""
    n = len(contigs)
    v = {f: np.zeros(n, np.int64) for f in A.FIELDS if f not in ("tied", "runs")}
    v["tied"], v["runs"] = np.full((n, A.TIED), -1, np.int64), np.zeros((n, A.RUNS), np.int64)
    j = {f: x.copy() for f, x in v.items()}
    j["gene"][:] = -1
    for k in range(n):
        tb = A.traceback(contigs[k], germs[own[k]])
        v["gene"][k], v["n_tied"][k], v["tied"][k, 0], v["del"][k] = own[k], 1, own[k], tb["dele"]
        for f in ("score", "seq_start", "seq_end", "germ_start", "germ_end", "matches", "mismatches", "ins", "opens", "n_runs"):
            v[f][k] = tb[f]
        v["runs"][k] = A.encode_runs(tb["ops"])
    return v, j


def test_cli_golden_condition():
    """The planting changes no V call, every planted codon lies well inside its contig's V hit, and the contigs show the designed
    classes.  A changed base moves the score of any alignment, and so S, by at most match + mismatch = 5; the scores against the records
    that are not planted do not move at all.  So a contig whose own V record is untouched keeps its call when every planted record, with
    that margin added, stays below the score of the contig's verbatim V window; the contigs of a planted clone (and those that are no
    verbatim window) are scored against every V record, with and without the planting."""
    fam = F.build()
    ids, seqs, recs, planted = planted_families()
    names, classes, germs, _, _ = parsed_records(recs)
    _, _, germs0, _, _ = parsed_records(fam.germline)
    vrec = [r for r, cl in enumerate(classes) if cl == "V"]
    changed = [r for r in vrec if germs[r] != germs0[r]]
    moved = {r: 5 * sum(a != b for a, b in zip(germs[r], germs0[r])) for r in changed}
    assert len(changed) == 10 and set(moved.values()) == {5, 10}
    who, _ = F.designed(fam, ids, seqs)
    hot = {who[c] for c in planted}
    full = [c for c, k in enumerate(who) if k is None or k in hot]
    rest = [c for c in range(len(seqs)) if c not in full]
    s1 = D.window_scores([seqs[c] for c in full], [germs[r] for r in vrec], A.DEFAULT)
    s0 = D.window_scores([seqs[c] for c in full], [germs0[r] for r in vrec], A.DEFAULT)
    for k in range(len(full)):
        assert np.flatnonzero(s1[k] == s1[k].max()).tolist() == np.flatnonzero(s0[k] == s0[k].max()).tolist() and s1[k].max() >= 40, full[k]
    sp = D.window_scores([seqs[c] for c in rest], [germs[r] for r in changed], A.DEFAULT)
    for k, c in enumerate(rest):
        verbatim = 2 * (300 - fam.rep.clones[who[c]].find(seqs[c]))           # the contig's own V window against its untouched record
        assert verbatim >= 40 and all(int(sp[k, q]) + moved[r] < verbatim for q, r in enumerate(changed)), c
    idx = sorted(planted)
    sub = [seqs[c] for c in idx]
    own = []
    for c in idx:
        row = s1[full.index(c)]
        assert (row == row.max()).sum() == 1
        own.append(vrec[int(row.argmax())])
        assert germs0[own[-1]] == fam.rep.v_germ[who[c]] and own[-1] in changed
    v, j = _v_hits(sub, germs, own)
    lim = M.mutation_limit([ids[c] for c in idx], sub)
    _, counts, _ = M.mutations(sub, v, None, j, lim, germs, [])
    seen = set()
    for k, c in enumerate(idx):
        kind, at, start = planted[c]
        gs, ge = int(v["germ_start"][k]), int(v["germ_end"][k])
        assert gs - 1 + 10 <= at and at + 3 + 10 <= ge, (c, kind, at, gs, ge)               # inside the hit, ten bases from its ends
        assert at - start + 3 <= lim[k]                                                       # below the limit: the junction's Cys codon
        want = dict(dict(v_r=0, v_s=0, v_stop=0, v_na=0), **WANT[kind])
        assert {f: int(counts[f][k]) for f in want} == want, (c, kind)
        seen.add(kind)
    assert seen == set(KINDS)


# ---- 4. the Python mirror ------------------------------------------------------------------------------------------------------------------
def test_python_mirror_of_the_abi():
    from vdjer_amd import _lib, annot, api
    assert ctypes.sizeof(_lib.MutRow) == 32 and ctypes.sizeof(_lib.MutInfo) == 72
    assert "vdjx_mutations" in _lib.SYMBOLS and "vdjx_mutations_layout" in _lib.SYMBOLS
    assert callable(api.Context.mutations) and api.Context.MUT_ROW.itemsize == 32
    ids = ["vjf_0_TGTGCA", "vjf_1_", "x", "vjf_3_ACG"]
    contigs = ["AATGTGCATT", "AATGTGCATT", "AATGTGCATT", "AAAAAAAACG"]
    assert annot.mutation_limit(ids, contigs).tolist() == [5, 10, 10, 10] == M.mutation_limit(ids, contigs).tolist()
    assert annot.mutation_limit(ids, contigs).dtype == np.int32
