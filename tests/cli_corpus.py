"""The command lines of tests/test_cli_options_cpu.py and tests/golden/make_golden_cli.py: every way `vdjer` refuses its options before
any GPU work, and the usage text.  A case is (name, argv after the program's name, extra environment); every case ends in parse() or in
main()'s checks right behind it, so none needs a GPU.

A command line whose options are all accepted is closed with `--gpus 0`: parse() returns 0 and main() refuses the run with one line
and no usage text -- which shows that the value was taken, not only that some line is absent."""
import os
import subprocess

BASE = ["--in", "reads.txt", "--chain", "IGH", "--ref-dir", "ref", "--ins", "175"]
STOP = ["--gpus", "0"]
U64 = 1 << 64

# a requirements row: (the flag and its value, what it needs, what else the command line must hold for this row to be the only fault)
LIN = ["--lineages", "l.tsv"]
REQUIRES = [
    (["--quant-boot", "8"], ["--quant", "q.tsv"], []),
    (["--quant-seed", "3"], ["--quant-boot", "8"], ["--quant", "q.tsv"]),
    (["--d-calls"], ["--airr", "a.tsv"], []),
    (["--isotypes", "i.tsv"], ["--cfa", "c.fa"], []),
    (["--lineage-dist", "0.2"], LIN, []),
    (["--lineage-model", "model.tsv"], LIN, []),
    (["--lineage-symmetry", "min"], ["--lineage-model", "model.tsv"], LIN),
    (["--lineage-threshold", "th.tsv"], LIN, []),
    (["--lineage-link", "complete"], LIN, []),
    (["--trees", "t.tsv"], LIN, []),
    (["--trees-nj", "nj.tsv"], LIN, []),
    (["--trees-newick", "nj.nwk"], ["--trees-nj", "nj.tsv"], LIN),
    (["--trees-mp", "mp.tsv"], LIN, []),
    (["--trees-mp-newick", "mp.nwk"], ["--trees-mp", "mp.tsv"], LIN),
    (["--tree-support", "8"], ["--trees", "t.tsv"], LIN),
    (["--tree-seed", "3"], ["--tree-support", "8"], LIN + ["--trees", "t.tsv"]),
    (["--diversity", "d.tsv"], LIN, ["--quant", "q.tsv"]),
    (["--diversity", "d.tsv"], ["--quant", "q.tsv"], LIN),
    (["--diversity-depth", "10"], ["--diversity", "d.tsv"], LIN + ["--clones", "cl.tsv"]),
    (["--diversity-boot", "10"], ["--diversity", "d.tsv"], LIN + ["--clones", "cl.tsv"]),
    (["--diversity-seed", "10"], ["--diversity", "d.tsv"], LIN + ["--clones", "cl.tsv"]),
    (["--v-regions", "regions.tsv"], ["--selection", "s.tsv"], []),
    (["--targeting", "model.tsv"], ["--selection", "s.tsv"], []),
    (["--selection-combine", "mean"], ["--selection", "s.tsv"], []),
    (["--selection-test", "st.tsv"], ["--selection", "s.tsv"], []),        # (no --v-regions either: that row's line follows)
    (["--selection-test", "st.tsv"], ["--v-regions", "regions.tsv"], ["--selection", "s.tsv"]),
    (["--consensus", "cs.tsv"], LIN, []),
    (["--consensus-min-freq", "0.5"], ["--consensus", "cs.tsv"], LIN),
    (["--targeting-class", "rs"], ["--targeting-model", "tm.tsv"], []),
    (["--targeting-min-sub", "5"], ["--targeting-model", "tm.tsv"], []),
    (["--targeting-min-mut", "5"], ["--targeting-model", "tm.tsv"], []),
    (["--targeting-counts", "tc.tsv"], ["--targeting-model", "tm.tsv"], []),
]

DIV = LIN + ["--quant", "q.tsv", "--diversity", "d.tsv"]
RANGES = [          # flag, lo, hi, what it needs
    ("--quant-boot", 1, 1024, ["--quant", "q.tsv"]),
    ("--tree-support", 1, 1024, LIN + ["--trees", "t.tsv"]),
    ("--diversity-depth", 1, 2147483647, DIV),
    ("--diversity-boot", 1, 4096, DIV),
    ("--targeting-min-sub", 1, 4294967295, ["--targeting-model", "tm.tsv"]),
    ("--targeting-min-mut", 1, 4294967295, ["--targeting-model", "tm.tsv"]),
]
SEEDS = [
    ("--quant-seed", ["--quant", "q.tsv", "--quant-boot", "8"]),
    ("--tree-seed", LIN + ["--trees", "t.tsv", "--tree-support", "8"]),
    ("--diversity-seed", DIV),
]
FRACTIONS = [
    ("--lineage-dist", LIN),
    ("--consensus-min-freq", LIN + ["--consensus", "cs.tsv"]),
]
WORDS = [
    ("--lineage-symmetry", ["avg", "min"], LIN + ["--lineage-model", "model.tsv"]),
    ("--lineage-link", ["single", "complete", "average"], LIN),
    ("--selection-combine", ["shared", "mean"], ["--selection", "s.tsv"]),
    ("--targeting-class", ["s", "rs"], ["--targeting-model", "tm.tsv"]),
]


def cases():
    """-> [(name, argv, env)] in a fixed order, names unique"""
    out = [("help", ["--help"], {}),
           ("help_behind_flags", BASE + ["--quant-boot", "0", "--help"], {}),
           ("help_as_a_value", ["--in", "--help"], {})]
    for k, (flag, need, rest) in enumerate(REQUIRES):
        out.append((f"needs_{k:02d}_{flag[0][2:]}_without_{need[0][2:]}", BASE + rest + flag, {}))
        out.append((f"needs_{k:02d}_{flag[0][2:]}_with_{need[0][2:]}", BASE + rest + need + flag + STOP, {}))
    for flag, lo, hi, need in RANGES:
        for v in (lo - 1, hi + 1, "x", "", "+1", "1.5", " 1"):
            out.append((f"range_{flag[2:]}_refuses_{v}", BASE + need + [flag, str(v)], {}))
        for v in (lo, hi):
            out.append((f"range_{flag[2:]}_takes_{v}", BASE + need + [flag, str(v)] + STOP, {}))
    for flag, need in SEEDS:
        for v in (-1, U64, "x", "", "0x10"):
            out.append((f"seed_{flag[2:]}_refuses_{v}", BASE + need + [flag, str(v)], {}))
        for v in (0, U64 - 1):
            out.append((f"seed_{flag[2:]}_takes_{v}", BASE + need + [flag, str(v)] + STOP, {}))
    for flag, need in FRACTIONS:
        for v in ("-0.1", "1.0001", "0.12345", "x", "", ".", "2", "10", "1e-1"):
            out.append((f"fraction_{flag[2:]}_refuses_{v}", BASE + need + [flag, v], {}))
        for v in ("0", "1", "0.0000", "1.0000", ".5", "0."):
            out.append((f"fraction_{flag[2:]}_takes_{v}", BASE + need + [flag, v] + STOP, {}))
    for flag, words, need in WORDS:
        for v in ("both", words[0].upper(), ""):
            out.append((f"word_{flag[2:]}_refuses_{v}", BASE + need + [flag, v], {}))
        for v in words:
            out.append((f"word_{flag[2:]}_takes_{v}", BASE + need + [flag, v] + STOP, {}))
    for v in ("", "1x", "-3", "1.0"):
        out.append((f"digits_total-count_refuses_{v}", BASE + ["--total-count", v], {}))
    out.append(("digits_total-count_takes_0012", BASE + ["--total-count", "0012"] + STOP, {}))
    out += [
        # the lookup's own quirks
        ("missing_value_of_the_last_flag", BASE + ["--quant"], {}),
        ("missing_value_of_an_unknown_last_flag", BASE + ["--bogus"], {}),
        ("d_calls_last_has_no_value", BASE + ["--airr", "a.tsv"] + STOP + ["--d-calls"], {}),
        ("d_calls_shifts_no_pair", BASE + ["--d-calls", "--airr", "a.tsv"] + STOP, {}),
        ("unknown_flag", BASE + ["--bogus", "1"] + STOP, {}),
        ("unknown_flag_then_a_refusal", BASE + ["--bogus", "1", "--quant-boot", "8"], {}),
        ("a_value_at_a_flag_position", BASE + ["q.tsv", "--quant"] + STOP, {}),
        ("jext_one_dash", BASE + ["-jext", "100"] + STOP, {}),
        ("jext_two_dashes", BASE + ["--jext", "100"] + STOP, {}),
        ("unlisted_flags", ["--in", "reads.txt", "--ins", "175", "--jc", "W", "--vf", "ref/v_index", "--jf", "ref/j_index", "--rms", "ref/v_region.fa", "--vdjf", "x.fa",
                            "--vr", "chr1:1-2", "--cr", "chr1:3-4"] + STOP, {}),
        ("unlisted_flags_after_ref_dir", BASE + ["--vf", "none"], {}),
        ("ref_dir_after_unlisted_flags", ["--in", "reads.txt", "--ins", "175", "--jc", "W", "--vf", "none", "--ref-dir", "ref"] + STOP, {}),
        ("every_plain_flag", BASE + ["--mf", "2", "--mq", "300", "--mcs", "-4.5", "--t", "2", "--am", "3", "--miw", "1", "--maw", "2", "--jc", "F", "--ws", "400",
                                     "--rf", "2", "--k", "25", "--vk", "14", "--mrs", "20", "--rs", "30", "--ms", "40", "--e0", "1", "--e1", "2", "--wo", "3",
                                     "--sample", "s1"] + STOP, {}),
        ("a_flag_given_twice_the_last_counts", BASE + ["--quant", "q.tsv", "--quant-boot", "0", "--quant-boot", "8"] + STOP, {}),
        ("a_flag_given_twice_the_last_is_bad", BASE + ["--quant", "q.tsv", "--quant-boot", "8", "--quant-boot", "0"], {}),
        # the checks that stay ordinary code
        ("nothing", [], {}),
        ("no_in", BASE[2:], {}),
        ("in_not_found", ["--in", "none.txt"] + BASE[2:], {}),
        ("no_ref_dir", ["--in", "reads.txt", "--chain", "IGH", "--ins", "175"], {}),
        ("ref_dir_not_found", ["--in", "reads.txt", "--chain", "IGH", "--ref-dir", "none", "--ins", "175"], {}),
        ("chain_unknown", ["--in", "reads.txt", "--chain", "IGX", "--ref-dir", "ref", "--ins", "175"], {}),
        ("jc_other", BASE + ["--jc", "X"], {}),
        ("no_ins", BASE[:6], {}),
        ("ins_zero", BASE[:6] + ["--ins", "0"], {}),
        ("vk_1", BASE + ["--vk", "1"], {}),
        ("vk_17", BASE + ["--vk", "17"], {}),
        ("vk_2", BASE + ["--vk", "2"] + STOP, {}),
        ("vk_16", BASE + ["--vk", "16"] + STOP, {}),
        ("cfa_not_found", BASE + ["--cfa", "none.fa"], {}),
        ("cfa_found", BASE + ["--cfa", "c.fa", "--isotypes", "i.tsv"] + STOP, {}),
        ("lineage_model_not_found", BASE + LIN + ["--lineage-model", "none.tsv"], {}),
        ("lineage_model_short", BASE + LIN + ["--lineage-model", "short.tsv"], {}),
        ("lineage_model_unread_without_lineages", BASE + ["--lineage-model", "none.tsv"], {}),
        ("v_regions_not_found", BASE + ["--selection", "s.tsv", "--v-regions", "none.tsv"], {}),
        ("v_regions_bad_interval", BASE + ["--selection", "s.tsv", "--v-regions", "bad_regions.tsv"], {}),
        ("v_regions_read", BASE + ["--selection", "s.tsv", "--v-regions", "regions.tsv", "--selection-test", "st.tsv"] + STOP, {}),
        ("targeting_not_found", BASE + ["--selection", "s.tsv", "--targeting", "none.tsv"], {}),
        ("targeting_short", BASE + ["--selection", "s.tsv", "--targeting", "short.tsv"], {}),
        ("targeting_read", BASE + ["--selection", "s.tsv", "--targeting", "model.tsv"] + STOP, {}),
        # main()'s checks behind parse()
        ("gpus_0", BASE + STOP, {}),
        ("gpus_257", BASE + ["--gpus", "257"], {}),
        ("quant_on_the_sharded_path", BASE + ["--quant", "q.tsv"], {"VDJX_FORCE_MGPU": "1"}),
        ("clones_on_the_sharded_path", BASE + ["--clones", "cl.tsv"], {"VDJX_FORCE_MGPU": "1"}),
        # several faults at once
        ("several_values_and_needs", BASE + ["--quant-boot", "0", "--quant-seed", "x", "--lineage-dist", "2", "--tree-support", "9999", "--tree-seed", "-1",
                                            "--consensus-min-freq", "7", "--targeting-class", "r", "--targeting-min-sub", "0"], {}),
        ("several_across_the_groups", ["--in", "none.txt", "--ins", "175", "--bogus", "1", "--isotypes", "i.tsv", "--cfa", "none.fa", "--diversity", "d.tsv",
                                       "--diversity-boot", "5000", "--selection-test", "st.tsv", "--selection-combine", "median", "--total-count", "x",
                                       "--lineage-link", "ward", "--vk", "40", "--jc", "Q"], {}),
        ("several_with_the_readers", BASE + LIN + ["--lineage-model", "short.tsv", "--lineage-symmetry", "max", "--selection", "s.tsv", "--v-regions", "none.tsv",
                                                   "--targeting", "none.tsv", "--trees-newick", "n.nwk", "--trees-mp-newick", "m.nwk", "--diversity-seed", "1"], {}),
        ("several_needs_only", BASE + ["--d-calls", "--quant-seed", "1", "--quant-boot", "2", "--lineage-threshold", "t", "--trees", "t", "--trees-nj", "t",
                                       "--trees-mp", "t", "--consensus", "c", "--targeting-counts", "c", "--v-regions", "regions.tsv", "--targeting", "model.tsv"], {}),
    ]
    names = [c[0] for c in out]
    assert len(set(names)) == len(names)
    return out


def write_inputs(d):
    """the files the cases name, in directory d (the read pool and reference of tests/test_quant_cpu._cli_inputs and the option files)"""
    with open(os.path.join(d, "reads.txt"), "w") as f:
        f.write("P r1 1 0 ACGTACGTAC IIIIIIIIII\nP r1 2 1 ACGTACGTAC IIIIIIIIII\n")
    os.makedirs(os.path.join(d, "ref"), exist_ok=True)
    for fn in ("v_index", "j_index"):
        with open(os.path.join(d, "ref", fn), "w") as f:
            f.write("1\t0\n")
    with open(os.path.join(d, "ref", "v_region.fa"), "w") as f:
        f.write(">v\nACGT\n")
    with open(os.path.join(d, "c.fa"), "w") as f:
        f.write(">IGHM*01\nACGTACGT\n")
    lines = []
    for m in range(1024):
        kmer = "".join("ACGT"[m >> s & 3] for s in (8, 6, 4, 2, 0))
        lines.append(kmer + "".join("\t0" if b == kmer[2] else f"\t{1 + (m + 3 * k) % 7}" for k, b in enumerate("ACGT")))
    with open(os.path.join(d, "model.tsv"), "w") as f:
        f.write("# a targeting model\n" + "\n".join(lines) + "\n")
    with open(os.path.join(d, "short.tsv"), "w") as f:
        f.write("\n".join(lines[:-1]) + "\n")
    with open(os.path.join(d, "regions.tsv"), "w") as f:
        f.write("# name cdr1 cdr2\nIGHV1-2*01 27 38 56 65\nIGHV3-23*01\t0\t0\t56\t65\n")
    with open(os.path.join(d, "bad_regions.tsv"), "w") as f:
        f.write("IGHV1-2*01 38 27 56 65\n")


def run(exe, d, argv, env):
    """one case in directory d -> (exit status, stderr, stdout); the VDJX_* variables of the caller's environment are not passed on"""
    e = {k: v for k, v in os.environ.items() if not k.startswith("VDJX_")}
    e.update(env)
    r = subprocess.run([exe] + argv, cwd=d, env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
    return r.returncode, r.stderr, r.stdout
