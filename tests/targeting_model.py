"""The targeting model of include/vdjx.h (vdjx_targeting_counts, vdjx_targeting_model, `vdjer --targeting-model`) restated in numpy and plain
Python.  The counts are integer: the device is tested against them bit for bit.  The finish does the C function's float64 operations in the
C function's order, one per statement, so every written weight is tested for equality.  The columns of a hit come from
tests/mutation_model.py and the genetic code from tests/annot_model.py, as tests/selection_model.py takes them.  Nothing here reads the
product."""
from __future__ import annotations

import numpy as np

from tests import annot_model as A
from tests import mutation_model as M

BASES = "ACGT"
INFO = ["contigs", "used", "truncated", "units", "positions", "obs_s", "obs_r", "opp_s", "opp_r", "batches"]
LEVELS = (5, 3, 1, 0)


def kmer(m):
    return "".join(BASES[m >> s & 3] for s in (8, 6, 4, 2, 0))


def index5(five):
    idx = 0
    for ch in five:
        idx = 4 * idx + BASES.index(ch)
    return idx


def codons(c, contig, v, limit, germs):
    """the classifiable codons of contig c's V hit, as vdjx_mutations and vdjx_selection define them -> (flags, gene, [(cod, germline codon,
    contig codon)]): all three bases in M columns below the limit, in three consecutive columns, all six characters ACGT"""
    lim = len(contig) if limit is None else int(limit[c])
    cols, flags, _ = M.columns(c, v, None, None)
    if not flags & M.F_V:
        return flags, -1, []
    gene = int(v["gene"][c])
    rec = germs[gene]
    where = {g: k for k, (reg, op, p, g) in enumerate(cols) if op == "M"}
    gs, ge = int(v["germ_start"][c]), int(v["germ_end"][c])
    out = []
    for cod in range(len(rec) // 3):
        gp = [3 * cod + 1, 3 * cod + 2, 3 * cod + 3]
        if gp[0] < gs or gp[2] > ge or any(g not in where for g in gp):
            continue
        ks = [where[g] for g in gp]
        if ks[1] != ks[0] + 1 or ks[2] != ks[1] + 1 or any(cols[k][2] - 1 >= lim for k in ks):
            continue
        gc, cc = "".join(rec[g - 1] for g in gp), "".join(contig[cols[k][2] - 1] for k in ks)
        if any(ch not in BASES for ch in gc + cc):
            continue
        out.append((cod, gc, cc))
    return flags, gene, out


def has_5mer(rec, p):
    """vdjx_selection's rule for the 0-based record position p: two bases on either side inside the RECORD, all ACGT"""
    return p >= 2 and p + 2 < len(rec) and all(ch in BASES for ch in rec[p - 2:p + 3])


def marks(contigs, v, limit, germs, group=None):
    """the bits every unit holds -> ({unit key: {p: set of base codes}}, {unit key: gene}, used, truncated)"""
    units, genes = {}, {}
    used = truncated = 0
    for c, s in enumerate(contigs):
        flags, gene, cods = codons(c, s, v, limit, germs)
        if not flags & M.F_V:
            truncated += bool(flags & M.F_TRUNC)
            continue
        used += 1
        key = (int(group[c]), gene) if group is not None and int(group[c]) >= 0 else ("own", c)
        bits = units.setdefault(key, {})
        genes[key] = gene
        rec = germs[gene]
        for cod, gc, cc in cods:
            if A.translate(gc) == "*":
                continue
            for b in range(3):
                p = 3 * cod + b
                if not has_5mer(rec, p):
                    continue
                here = bits.setdefault(p, set())
                here.add(BASES.index(gc[b]))
                if cc[b] != gc[b] and A.translate(gc[:b] + cc[b] + gc[b + 1:]) != "*":
                    here.add(BASES.index(cc[b]))
    return units, genes, used, truncated


def counts(contigs, v, limit, germs, group=None, per_batch=1 << 18):
    """the model of vdjx_targeting_counts -> (uint64[2, 2, 1024, 4], info dict)"""
    units, genes, used, truncated = marks(contigs, v, limit, germs, group)
    out = np.zeros((2, 2, 1024, 4), np.uint64)
    positions = 0
    for key, bits in units.items():
        rec = germs[genes[key]]
        for p, here in bits.items():
            positions += 1
            m = index5(rec[p - 2:p + 3])
            cod, b = divmod(p, 3)
            gc = rec[3 * cod:3 * cod + 3]
            aa = A.translate(gc)
            for x in range(4):
                if BASES[x] == gc[b]:
                    continue
                ma = A.translate(gc[:b] + BASES[x] + gc[b + 1:])
                if ma == "*":
                    continue
                k = int(ma != aa)
                out[1, k, m, x] += 1
                if x in here:
                    out[0, k, m, x] += 1
    tot = [[int(out[a, k].sum()) for k in range(2)] for a in range(2)]
    info = dict(contigs=len(contigs), used=used, truncated=truncated, units=len(units), positions=positions, obs_s=tot[0][0], obs_r=tot[0][1],
                opp_s=tot[1][0], opp_r=tot[1][1], batches=-(-len(units) // per_batch))
    return out, info


def model(cnt, cls="s", min_sub=50, min_mut=500):
    """the model of vdjx_targeting_model -> (weight uint32[1024, 4], level uint8[1024, 2]); Python floats are float64 and every statement
    below is one operation of the C function"""
    cnt = np.asarray(cnt, np.uint64)
    obs = [[int(cnt[0, 0, m, x]) + (int(cnt[0, 1, m, x]) if cls == "rs" else 0) for x in range(4)] for m in range(1024)]
    opp = [[int(cnt[1, 0, m, x]) + (int(cnt[1, 1, m, x]) if cls == "rs" else 0) for x in range(4)] for m in range(1024)]
    inner = lambda m: m >> 2 & 63
    centre = lambda m: m >> 4 & 3
    sets = {5: lambda m: [m], 3: lambda m: [q for q in range(1024) if inner(q) == inner(m)], 1: lambda m: [q for q in range(1024) if centre(q) == centre(m)],
            0: lambda m: list(range(1024))}
    memo = {}

    def sums(lv, m):
        """(a[4], o, p) of 5-mer m's set at a level"""
        key = (lv, m if lv == 5 else inner(m) if lv == 3 else centre(m) if lv == 1 else 0)
        if key not in memo:
            qs = sets[lv](m)
            a = [sum(obs[q][x] for q in qs) for x in range(4)]
            memo[key] = (a, sum(a), sum(sum(opp[q]) for q in qs))
        return memo[key]

    _, o0, p0 = sums(0, 0)
    level = np.zeros((1024, 2), np.uint8)
    mut = []
    for m in range(1024):
        for lv in LEVELS:
            _, o, p = sums(lv, m)
            if lv == 0 or (o >= min_mut and p > 0):
                break
        level[m, 1] = lv
        mut.append(1.0 if o0 == 0 or p0 == 0 else float(o) / float(p))
    z = 0.0
    for m in range(1024):
        z = z + mut[m]
    weight = np.zeros((1024, 4), np.uint32)
    for m in range(1024):
        c = centre(m)
        for lv in LEVELS:
            a, tot, _ = sums(lv, m)
            if lv == 0:
                a, tot = [int(x != c) for x in range(4)], 3
            if lv == 0 or tot >= min_sub:
                break
        level[m, 0] = lv
        mz = mut[m] / z
        for x in range(4):
            if x == c:
                continue
            s = float(a[x]) / float(tot)
            t = mz * s
            scaled = t * 1e9
            r = float(np.rint(scaled))
            weight[m, x] = 1 if r < 1.0 else int(r)
    return weight, level


def level_counts(level):
    """per table (substitution, mutability) the 5-mers on level 5, 3, 1, 0 -> [[n5, n3, n1, n0]] * 2"""
    return [[int((level[:, t] == lv).sum()) for lv in LEVELS] for t in range(2)]


def model_text(sample, cls, min_sub, min_mut, info, weight, level):
    """the file `vdjer --targeting-model` writes"""
    lc = level_counts(level)
    out = [f"# targeting model of {sample}: class {cls}, min_sub {min_sub}, min_mut {min_mut}",
           f"# {info['units']} units, {info['positions']} positions, observed {info['obs_s']} S {info['obs_r']} R, opportunities {info['opp_s']} S {info['opp_r']} R",
           "# substitution levels 5/3/1/0: %d/%d/%d/%d 5-mers" % tuple(lc[0]), "# mutability levels 5/3/1/0: %d/%d/%d/%d 5-mers" % tuple(lc[1])]
    out += [kmer(m) + "".join(f"\t{int(x)}" for x in weight[m]) for m in range(1024)]
    return "\n".join(out) + "\n"


def counts_text(cnt, level):
    """the file `vdjer --targeting-counts` writes"""
    head = ["kmer"] + [f"{a}_{k}_{x}" for a in ("obs", "opp") for k in "sr" for x in "acgt"] + ["sub_level", "mut_level"]
    out = ["\t".join(head)]
    for m in range(1024):
        out.append("\t".join([kmer(m)] + [str(int(cnt[a, k, m, x])) for a in range(2) for k in range(2) for x in range(4)] + [str(int(level[m, 0])), str(int(level[m, 1]))]))
    return "\n".join(out) + "\n"


def summary_line(info, cls, level):
    lc = level_counts(level)
    return ("targeting model: %d contigs, %d used, %d units, %d positions, %d S, %d R, class %s, substitution levels %d/%d/%d/%d, mutability levels %d/%d/%d/%d, %d batches"
            % (info["contigs"], info["used"], info["units"], info["positions"], info["obs_s"], info["obs_r"], cls, *lc[0], *lc[1], info["batches"]))
