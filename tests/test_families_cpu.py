"""The e2e_families golden without a GPU: the committed contigs meet the conditions that make tests/test_gpu_tables.py non-vacuous (asserted
from the recipe's designed gene names and the junction text in the contig ids, no aligner involved), the recipe's design holds, and the FASTA
files it writes read back as designed through vdjer_amd/annot.py's reader and name rules."""
from tests import families as F
from tests import golden_util as G
from tests import isotype_model as I
from vdjer_amd import annot


def test_golden_meets_the_conditions():
    fam = F.build()
    info = G.manifest()[F.TAG]
    ids, seqs = F.golden_contigs(G.text(f"{F.TAG}.contigs.fa.gz"))
    assert len(ids) == info["contigs"] == len(set(ids)) and {len(s) for s in seqs} == {F.WINDOW_SPAN}
    who, cond = F.designed(fam, ids, seqs)
    F.check_conditions(cond)
    assert cond == info["conditions"]
    # every contig is the window the recipe designed for one clone, every clone has one
    assert cond["verbatim"] == len(ids) == len(set(who)) == len(fam.clones) == info["clones"]
    assert sorted(seqs) == sorted(F.windows(fam))
    assert (info["seed"], info["copies"], info["step"], info["flags"]) == (F.SEED, F.COPIES, F.STEP, F.FLAGS)
    # 65 distinct keys are what it takes for the key tables of clones_table / lineage_run (64 to begin with) to grow
    assert cond["groups"] >= 65 and cond["eligible"] == len(ids) - 1 and cond["lineages_at_005"] > cond["lineages"]


def test_recipe_design():
    fam = F.build()
    F.check_design(fam)
    assert F.build() is fam and F.build.__wrapped__().rep.clones == fam.rep.clones           # deterministic from the seed
    pool = F.pool(fam)
    assert pool.n_pairs == G.manifest()[F.TAG]["pairs"] and pool.secondary.shape[0] == 0
    # the D records cut from cores lie in their clones' cores, the duplicate is one of them, the lone clone has no J record
    assert sum(bool(c.d_name) for c in fam.clones) == 6 and all(fam.d_cuts[c.d_name] in c.core for c in fam.clones if c.d_name)
    assert len(fam.d_cuts) == 12 and len(set(fam.d_cuts.values())) == 11
    assert [c.j_names for c in fam.clones].count([]) == 1 and not fam.clones[-1].j_names


def test_fasta_files_read_back_as_designed(tmp_path):
    fam = F.build()
    F.write_ref_dir(fam, str(tmp_path / "ref"))
    F.write_cfa(fam, str(tmp_path / "c.fa"))
    raw = annot.read_fasta(str(tmp_path / "ref" / "ig_vdj.fa"))
    parsed = [annot.parse_record(h, s) for h, s in raw]
    text = (tmp_path / "ref" / "ig_vdj.fa").read_text()
    assert any(h.count("|") >= 2 for h, _ in raw) and any(s != s.upper() for _, s in raw) and max(len(l) for l in text.splitlines()) == 300
    assert sum(len(l) == 60 for l in text.splitlines()) >= 8                                  # (wrapped records)
    assert [(n, s) for n, _, s in parsed] == [(annot.parse_name(h), s) for h, s in F.records(fam)]
    by_name = {n: (cls, s) for n, cls, s in parsed}
    assert len(by_name) == len(parsed)
    for k, c in enumerate(fam.clones):
        for name in c.v_names:
            assert by_name[name] == ("V", fam.rep.v_germ[k]), name
        for name in c.j_names:
            assert by_name[name] == ("J", fam.rep.j_germ[k][:F.J_RECORD]), name
        # the gene strings written down by hand are what both Python restatements of get_vq_gene make of the names
        assert annot.vq_gene(c.v_names) == I.vq_gene(c.v_names) == c.vgene, c.v_names
        assert annot.vq_gene(c.j_names) == I.vq_gene(c.j_names) == c.jgene, c.j_names
    assert sorted(n for n, (cls, _) in by_name.items() if cls == "D") == sorted(fam.d_cuts) and all(by_name[n][1] == s for n, s in fam.d_cuts.items())
    assert not fam.rep.j_germ[-1][:F.J_RECORD] in {s for _, s in by_name.values()}
    const = [(annot.parse_name(h), annot.clean_seq(s)) for h, s in annot.read_fasta(str(tmp_path / "c.fa"))]
    assert const == fam.constant and [n for n, _ in const] == F.CONST_NAMES
