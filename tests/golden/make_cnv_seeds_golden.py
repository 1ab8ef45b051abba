"""Generate tests/golden/cnv_seeds.json from the REAL reference (build container only):

    python tests/golden/make_cnv_seeds_golden.py [the reference's src/ directory, default /root/reference/src]

It imports the unmodified reference module cnv_seed, calls run_seeding with all three thresholds set (the reference fails with
UnboundLocalError otherwise) on small hand-made copy-number files, and records per case the input text and its extension, the
output bed - or the exception the reference ends with - and, once, the centromere rows and the chromosome sizes the reference
read (its annotations/GRCh38_centromere.bed and global_names.chr_sizes).  Nothing of the reference's program text is stored.
tests/test_cnv_seeds.py holds cnv.find_seeds against the file, text for text."""
import argparse
import contextlib
import io
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
GAIN, MIN_SEED_SIZE, MAX_SEG_GAP = 6.0, 99999, 300001


def cns(rows):
    """rows of (chrom, start, end, log2) -> a CNVkit .cns text."""
    head = "chromosome\tstart\tend\tgene\tlog2\tdepth\tprobes\tweight\n"
    return head + "".join("%s\t%d\t%d\t-\t%r\t%r\t%d\t%d\n" % (c, a, b, l, 10.0 * 2 ** l, (b - a) // 1000, (b - a) // 1000) for c, a, b, l in rows)


def bed(rows):
    """rows of (chrom, start, end, cn) -> the .bed flavour."""
    return "".join("%s\t%d\t%d\t%r\n" % row for row in rows)


def cases():
    """name -> (extension, text).  hg38: chr1's centromere rows span 121 700 000 - 125 100 000, chr21's 10 900 000 - 13 000 000."""
    L8, L65, L2 = 2.0, 1.7004397181410922, 0.0              # log2 of CN 8, 6.5 and 2
    T = {}
    T["p_arm"] = (".cns", cns([("chr1", 0, 10_000_000, L2), ("chr1", 10_000_000, 10_200_000, L8), ("chr1", 10_200_000, 121_000_000, L2)]))
    T["q_arm"] = (".cns", cns([("chr1", 126_000_000, 200_000_000, L2), ("chr1", 200_000_000, 200_150_000, L8), ("chr1", 200_150_000, 248_000_000, L2)]))
    T["both_arms_bed"] = (".bed", bed([("chr1", 5_000_000, 5_400_000, 9.5), ("chr1", 100_000_000, 130_000_000, 2.0), ("chr1", 150_000_000, 150_250_000, 12.0),
                                       ("chr2", 1_000_000, 1_120_000, 6.0), ("chr2", 200_000_000, 200_090_000, 30.0)]))
    for gap in (300001, 300002):
        T["gap_%d" % gap] = (".cns", cns([("chr3", 1_000_000, 1_060_000, L8), ("chr3", 1_060_000, 1_060_000 + gap, L2), ("chr3", 1_060_000 + gap, 1_120_000 + gap, L8)]))
    for length in (99998, 99999, 100000):
        T["length_%d" % length] = (".bed", bed([("chr4", 2_000_000, 2_000_000 + length // 2, 7.0), ("chr4", 2_000_000 + length // 2, 2_000_000 + length, 8.0)]))
    T["long_seed_between_gain_and_1p2_gain"] = (".cns", cns([("chr5", 10_000_000, 15_000_002, L65), ("chr5", 20_000_000, 25_000_001, L65), ("chr6", 10_000_000, 15_000_002, L8)]))
    T["arm_at_cn4_raises_the_cutoff"] = (".bed", bed([("chr21", 0, 6_000_000, 4.0), ("chr21", 6_000_000, 6_200_000, 7.0), ("chr21", 6_200_000, 6_300_000, 4.0),
                                                      ("chr21", 6_300_000, 6_500_000, 9.0), ("chr21", 6_500_000, 10_000_000, 3.0), ("chr21", 20_000_000, 20_200_000, 7.0)]))
    T["cutoff_splits_a_chain"] = (".bed", bed([("chr7", 1_000_000, 1_200_000, 8.0), ("chr7", 1_200_000, 6_000_000, 6.2), ("chr7", 6_000_000, 6_200_000, 8.0),
                                               ("chr7", 6_300_000, 6_450_000, 8.0)]))
    T["dropped_segment_quirk"] = (".bed", bed([("chr8", 1_000_000, 1_050_000, 8.0), ("chr8", 1_050_000, 7_000_000, 6.2), ("chr8", 7_000_000, 7_200_000, 8.0)]))
    T["no_seed"] = (".cns", cns([("chr9", 0, 1_000_000, L2), ("chr9", 1_000_000, 1_050_000, L8), ("chr9", 1_050_000, 40_000_000, L2), ("chrX", 1_000_000, 1_090_000, L8)]))
    T["no_gain_at_all"] = (".cns", cns([("chr9", 0, 40_000_000, L2), ("chr10", 0, 30_000_000, 0.5)]))
    return T


def main(ref_src):
    sys.path.insert(0, ref_src)
    import cnv_seed            # the reference's module, as it is
    import global_names
    with open(os.path.join(ref_src, "annotations", "GRCh38_centromere.bed")) as fp:
        centromeres = [line.split() for line in fp if line.strip()]
    out = {"made_by": "cnv_seed.run_seeding(args) of the reference with gain, min_seed_size and max_seg_gap set", "gain": GAIN, "min_seed_size": MIN_SEED_SIZE,
           "max_seg_gap": MAX_SEG_GAP, "centromeres": centromeres, "chrom_sizes": {row[0]: global_names.chr_sizes[row[0]] for row in centromeres}, "cases": {}}
    with tempfile.TemporaryDirectory() as d:
        for name, (ext, text) in cases().items():
            src, dst = os.path.join(d, name + ext), os.path.join(d, name + "_seeds_out.bed")
            with open(src, "w") as fp:
                fp.write(text)
            args = argparse.Namespace(cn_seg=src, gain=GAIN, min_seed_size=MIN_SEED_SIZE, max_seg_gap=MAX_SEG_GAP, out=dst)
            case = {"extension": ext, "input": text}
            try:
                with contextlib.redirect_stdout(io.StringIO()):
                    cnv_seed.run_seeding(args)
                with open(dst) as fp:
                    case["seeds"] = fp.read()
            except Exception as e:                                # (what the reference does with such a file)
                case["reference_raises"] = type(e).__name__
            out["cases"][name] = case
    with open(os.path.join(HERE, "cnv_seeds.json"), "w") as fp:
        json.dump(out, fp, indent=1)
        fp.write("\n")
    for name, case in out["cases"].items():
        print(name, repr(case.get("seeds", case.get("reference_raises"))))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "/root/reference/src")
