#!/usr/bin/env python3
"""`CoRAL.py reconstruct` with the MI355X graph build (same flags as /root/reference/src/CoRAL.py:80-109).

    python -m coral_amd.CoRAL reconstruct --lr_bam x.bam --cnv_seed seeds.bed --cn_seg cn.bed --output_prefix out \\
        --skip_cycle_decomp

The `reconstruct` mode and the `hsr` mode (§8(f) item 3) run on the MI355X path, and so do `index`, `qc`
(the reference's scripts/report_nanopore_qc.py, from one decode of the aligned BAM or, with --fastq, from the reads' FASTQ), `pileup` (the bases per position of
regions, pysam's count_coverage as a table) and `depth` (read depth per fixed-size bin of every contig, the table a copy-number
caller starts from), `fastq` (selected reads as FASTQ, by regions or read names), `view` (the same selection as a BAM file of
the records themselves, with its index on request) and `sort` (the kept records in coordinate order as a BAM file, with its
index on request: lines 42-50 of the reference's scripts/align_nanopore_reads.sh from one decode) and `import` (the mapper's
SAM text as the BAM file `sort` opens: line 38 of that script) and `cnv` (the .cns of segmented copy number and the seed
intervals that `reconstruct` starts from: scripts/call_cnvs.sh and the seed mode, from the binned depth) and `kmers` (the
reference genome's repetitive k-mers, the list the mapper takes with -W: lines 29-30 of that script) and `composition` (the
reference genome's G/C, A/T and soft-masked bases per depth bin, which `cnv --ref / --composition` corrects the GC bias with: the
gc and rmask columns of the reference table of scripts/call_cnvs.sh) and `filter` (the reads of a FASTQ file that are long and
good enough, written as they were read: the "Quality filter reads" that scripts/report_nanopore_qc.py announces) and `sketch` (the
reference genome's window minimizers sorted by hash, the mapper's first stage: line 34 of scripts/align_nanopore_reads.sh); the other modes of the
reference (seed, plot, cycle2bed) are untouched and are delegated to the reference's own modules when they are
importable (set CORAL_REFERENCE_SRC to the reference's src/ directory).  The cycle-decomposition step after the graph build is the
reference's (Gurobi); it runs on the object this module returns.
"""
import argparse
import os
import sys

# host side = one thread + a few native workers: keep the per-core OpenMP / BLAS pools from spinning (coral_amd/hostpools.py)
for _v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
    os.environ.setdefault(_v, "1" if _v.startswith("OPENBLAS") else "4")
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")      # (ROCm's default of 4 hardware queues makes the decoder's and the build's streams share queues)


def print_args(args_dict):
    for key, value in vars(args_dict).items():
        print(f"{key}: {value}")
    print()


def add_filter_arguments(p):
    """--filter_*: the record filter of the decode (bam.RecordFilter), what `samtools view -q / -f / -F` and a length test in
    front of the file would do; integers in any base, 0 = no test."""
    any_int = lambda x: int(x, 0)
    p.add_argument("--filter_min_mapq", help="Drop reads of a lower mapping quality while the bam file is decoded.", type=any_int, default=0)
    p.add_argument("--filter_min_length", help="Drop reads with a shorter stored sequence.", type=any_int, default=0)
    p.add_argument("--filter_require_flags", help="Drop reads that lack any of these flag bits.", type=any_int, default=0)
    p.add_argument("--filter_exclude_flags", help="Drop reads with any of these flag bits.", type=any_int, default=0)


def record_filter_of(args):
    """The bam.RecordFilter of an argument object (one without the --filter_* attributes: no filter)."""
    from coral_amd import bam
    return bam.record_filter_from_args(args)


def build_parser():
    parser = argparse.ArgumentParser(description="Long-read amplicon reconstruction pipeline and associated utilities.")
    sub = parser.add_subparsers(dest="mode", help="Select mode.")
    rp = sub.add_parser("reconstruct", help="Reconstruct focal amplifications")
    rp.add_argument("--lr_bam", help="Sorted indexed (long read) bam file.", required=True)
    rp.add_argument("--cnv_seed", help="Bed file of CNV seed intervals.", required=True)
    rp.add_argument("--output_prefix", help="Prefix of output files.", required=True)
    rp.add_argument("--cn_seg", help="Long read segmented whole genome CN calls (.bed or CNVkit .cns file).", required=True)
    rp.add_argument("--output_bp", help="If specified, only output the list of breakpoints.", action='store_true')
    rp.add_argument("--skip_cycle_decomp", help="If specified, only reconstruct and output the breakpoint graph for all amplicons.",
                    action='store_true')
    rp.add_argument("--output_all_path_constraints", help="If specified, output all path constraints in *.cycles file.",
                    action='store_true')
    rp.add_argument("--min_bp_support", help="Ignore breakpoints with less than (min_bp_support * normal coverage) long read support.",
                    type=float, default=1.0)
    rp.add_argument("--cycle_decomp_alpha", help="Parameter used to balance CN weight and path constraints in greedy cycle extraction.",
                    type=float, default=0.01)
    rp.add_argument("--cycle_decomp_time_limit", help="Maximum running time (in seconds) reserved for integer program solvers.",
                    type=int, default=7200)
    rp.add_argument("--cycle_decomp_threads", help="Number of threads reserved for integer program solvers.", type=int)
    rp.add_argument("--postprocess_greedy_sol", help="Postprocess the cycles/paths returned in greedy cycle extraction.",
                    action='store_true')
    rp.add_argument("--log_fn", help="Name of log file.")
    rp.add_argument("--device", help="GPU to use (MI355X build only option).", default="cuda:0")
    hp = sub.add_parser("hsr", help="Detect possible integration points of ecDNA HSR amplifications.")     # CoRAL.py:112-120
    hp.add_argument("--lr_bam", help="Sorted indexed long read bam file.", required=True)
    hp.add_argument("--cycles", help="AmpliconSuite-formatted cycles file", required=True)
    hp.add_argument("--cn_seg", help="Long read segmented whole genome CN calls (.bed or CNVkit .cns file).", required=True)
    hp.add_argument("--output_prefix", help="Prefix of output file name.", required=True)
    hp.add_argument("--normal_cov", help="Estimated diploid coverage.", required=True)
    hp.add_argument("--bp_match_cutoff", help="Breakpoint matching cutoff.", type=int, default=100)
    hp.add_argument("--bp_match_cutoff_clustering", help="Crude breakpoint matching cutoff for clustering.", type=int, default=2000)
    hp.add_argument("--device", help="GPU to use (MI355X build only option).", default="cuda:0")
    ip = sub.add_parser("index", help="Write the BAI index of a sorted bam file (x.bam.bai), from one decode of it.")
    ip.add_argument("--lr_bam", help="Sorted (long read) bam file.", required=True)
    ip.add_argument("--index", help="Name of the index file (default: <lr_bam>.bai).")
    ip.add_argument("--device", help="GPU to use ('cpu': the host pipeline).", default="cuda:0")
    qp = sub.add_parser("qc", help="Report read length and base quality statistics of a (long read) bam file, or of the reads' FASTQ file.")
    qp.add_argument("--lr_bam", help="(Long read) bam file.")
    qp.add_argument("--fastq", help="FASTQ file of the reads, in place of --lr_bam (a name ending in .gz is inflated on the host).")
    qp.add_argument("--chunk_bytes", help="With --fastq: bytes of the FASTQ file per piece.", type=int, default=64 << 20)
    qp.add_argument("--output_dir", help="Where to write the summary and the plots.", required=True)
    qp.add_argument("--device", help="GPU to use ('cpu': the host pipeline).", default="cuda:0")
    qp.add_argument("--no_plots", help="If specified, write no histogram images.", action='store_true')
    pp = sub.add_parser("pileup", help="Count the A, C, G and T bases at every position of regions of a (long read) bam file.")
    pp.add_argument("--lr_bam", help="Sorted (long read) bam file.", required=True)
    where = pp.add_mutually_exclusive_group(required=True)
    where.add_argument("--region", help="chr:start-stop (0-based, half-open); may be given several times.", action="append")
    where.add_argument("--bed", help="Bed file of regions.")
    pp.add_argument("--min_base_quality", help="Count only bases of at least this quality.", type=int, default=0)
    pp.add_argument("--read_callback", help="'all' leaves out unmapped, secondary, QC-fail and duplicate reads.",
                    choices=("all", "nofilter"), default="nofilter")
    pp.add_argument("--output", help="Name of the output file (tab-separated).", required=True)
    pp.add_argument("--device", help="GPU to use ('cpu': the host pipeline).", default="cuda:0")
    dp = sub.add_parser("depth", help="Sum read depth into fixed-size bins along every contig of a (long read) bam file.")
    dp.add_argument("--lr_bam", help="(Long read) bam file.", required=True)
    dp.add_argument("--output", help="Name of the output file (tab-separated, CNVkit's .cnn columns).", required=True)
    dp.add_argument("--bin_size", help="Bases per bin.", type=int, default=1000)
    dp.add_argument("--min_mapq", help="Leave out reads of a lower mapping quality.", type=int, default=0)
    dp.add_argument("--exclude_flags", help="Leave out reads with any of these flag bits (default: unmapped, secondary, QC-fail, duplicate).",
                    type=int, default=0x704)
    dp.add_argument("--no_deletions", help="If specified, deleted reference bases (D) do not count as covered.", action='store_true')
    dp.add_argument("--device", help="GPU to use ('cpu': the host pipeline).", default="cuda:0")
    fp = sub.add_parser("fastq", help="Write selected reads of a (long read) bam file as FASTQ, from one decode of it.")
    fp.add_argument("--lr_bam", help="(Long read) bam file.", required=True)
    fp.add_argument("--region", help="chr:start-stop (0-based, half-open): only reads that overlap it; may be given several times.", action="append")
    fp.add_argument("--names_file", help="File of read names, one per line: only these reads.")
    fp.add_argument("--reads_exclude_flags", help="Leave out records with any of these flag bits (default: secondary, supplementary).",
                    type=lambda x: int(x, 0), default=0x900)
    fp.add_argument("--stream", help="Write each batch's text to the file while the input is decoded on the GPU (--device; cuda:0 with --device cpu): "
                    "bounded host memory, for every read of a file of any size.", action='store_true')
    fp.add_argument("--output", help="Name of the FASTQ file.", required=True)
    fp.add_argument("--device", help="GPU to use ('cpu': the host pipeline).", default="cuda:0")
    vp = sub.add_parser("view", help="Write selected records of a (long read) bam file as a BAM file, from one decode of it.")
    vp.add_argument("--lr_bam", help="(Long read) bam file.", required=True)
    vp.add_argument("--region", help="chr:start-stop (0-based, half-open): only records that overlap it; may be given several times.", action="append")
    vp.add_argument("--names_file", help="File of read names, one per line: only the records of these reads.")
    vp.add_argument("--reads_exclude_flags", help="Leave out records with any of these flag bits (default: none).",
                    type=lambda x: int(x, 0), default=0)
    vp.add_argument("--level", help="Compression level of the BAM file, 0..9.", type=int, default=1)
    vp.add_argument("--index", help="If specified, also write the BAI index (<output>.bai).", action='store_true')
    vp.add_argument("--gpu_compress", help="Deflate the BAM file's BGZF blocks on the GPU (--device; cuda:0 with --device cpu) instead of on the host; --level must be 1.", action='store_true')
    vp.add_argument("--stream", help="Write the BAM file while the input is decoded, its BGZF blocks deflated on the GPU (--device; cuda:0 with --device cpu): "
                    "bounded host memory, for a file of any size; implies --gpu_compress and --level 1.", action='store_true')
    vp.add_argument("--output", help="Name of the BAM file.", required=True)
    vp.add_argument("--device", help="GPU to use ('cpu': the host pipeline).", default="cuda:0")
    sp = sub.add_parser("sort", help="Write the records of a (long read) bam file in coordinate order as a BAM file, from one decode of it.")
    sp.add_argument("--lr_bam", help="(Long read) bam file, in any order.", required=True)
    sp.add_argument("--reads_exclude_flags", help="Leave out records with any of these flag bits (default: none).",
                    type=lambda x: int(x, 0), default=0)
    sp.add_argument("--level", help="Compression level of the BAM file, 0..9.", type=int, default=1)
    sp.add_argument("--index", help="If specified, also write the BAI index (<output>.bai).", action='store_true')
    sp.add_argument("--gpu_compress", help="Deflate the BAM file's BGZF blocks on the GPU (--device; cuda:0 with --device cpu) instead of on the host; --level must be 1.", action='store_true')
    sp.add_argument("--stream", help="Spill each batch's sorted run to disk and merge the runs on the GPU (--device; cuda:0 with --device cpu): "
                    "bounded host memory, for a file of any size; implies --gpu_compress and --level 1.", action='store_true')
    sp.add_argument("--tmp_dir", help="With --stream: directory of the spill file <output's name>.runs.tmp (default: the output's directory).")
    sp.add_argument("--output", help="Name of the sorted BAM file.", required=True)
    sp.add_argument("--device", help="GPU to use ('cpu': the host pipeline).", default="cuda:0")
    mp = sub.add_parser("import", help="Write a mapper's SAM text as a BAM file, its records encoded on the GPU.")
    mp.add_argument("--sam", help="SAM text; '-' reads standard input, so that the mapper pipes into it.", required=True)
    mp.add_argument("--output", help="Name of the BAM file.", required=True)
    mp.add_argument("--level", help="With --device cpu: compression level of the BAM file, 0..9 (the GPU path deflates on the device at its one setting).",
                    type=int, default=1)
    mp.add_argument("--gpu_compress", help="With --device cpu: deflate the BAM file's BGZF blocks on the GPU (cuda:0) instead of on the host; --level must be 1.",
                    action='store_true')
    mp.add_argument("--device", help="GPU to use ('cpu': the host's rule book, one thread, the whole text in memory).", default="cuda:0")
    cp = sub.add_parser("cnv", help="Call segmented copy number (.cns) and seed intervals from a sorted bam file or its binned depth.")
    source = cp.add_mutually_exclusive_group(required=True)
    source.add_argument("--lr_bam", help="Sorted (long read) bam file.")
    source.add_argument("--depth", help="Binned-depth table written by the depth mode, in place of the bam file.")
    cp.add_argument("--output", help="Name of the output file (CNVkit's .cns columns).", required=True)
    cp.add_argument("--reference_cnn", help="Binned-depth table of a normal sample with the same bins (the depth mode's output).")
    cp.add_argument("--bin_size", help="Bases per bin (with --lr_bam).", type=int, default=1000)
    cp.add_argument("--levels", help="Dyadic scales of the Haar segmenter, 1..20.", type=int, default=5)
    cp.add_argument("--fdr_q", help="False discovery rate of the breakpoint test, in (0, 1).", type=float, default=1e-4)
    cp.add_argument("--seeds", help="Also write the CNV seed intervals (the reference's seed mode) to this bed file; needs --centromeres.")
    cp.add_argument("--centromeres", help="Centromere bed file (chrom, start, end, band; a p row and a q row per contig).")
    cp.add_argument("--chrom_sizes", help="Two-column file of contig lengths for --seeds (default: the bam file's header, or the depth table).")
    cp.add_argument("--gain", help="Minimum CN of a seed segment.", type=float, default=6.0)
    cp.add_argument("--min_seed_size", help="Minimum summed length of a seed.", type=int, default=99999)
    cp.add_argument("--max_seg_gap", help="Maximum gap between the segments of one seed.", type=int, default=300001)
    cp.add_argument("--device", help="GPU to use ('cpu': the host backend).", default="cuda:0")
    comp = cp.add_mutually_exclusive_group()
    comp.add_argument("--ref", help="Reference genome, FASTA: its composition is counted at the depth's bin size, for the GC correction and the uncalled-base mask.")
    comp.add_argument("--composition", help="Per-bin composition table written by the composition mode, in place of --ref.")
    cp.add_argument("--gc_strata", help="With --ref / --composition: steps of the GC fraction, 1..1000.", type=int, default=100)
    cp.add_argument("--gc_min_bins", help="With --ref / --composition: bins a stratum's bias is the median of (neighbouring strata are pooled up to it).", type=int, default=256)
    cp.add_argument("--min_called", help="With --ref / --composition: smallest fraction of a bin's bases that are A, C, G or T, in [0, 1].", type=float, default=0.5)
    kp = sub.add_parser("kmers", help="Count a reference's k-mers and write the repetitive ones (the mapper's -W list) from its FASTA file.")
    kp.add_argument("--ref", help="Reference genome, FASTA (a name ending in .gz is inflated on the host).", required=True)
    kp.add_argument("--output", help="Name of the output file (KMER<tab>COUNT lines).", required=True)
    kp.add_argument("--k", help="K-mer size, 1..16.", type=int, default=15)
    cut = kp.add_mutually_exclusive_group()
    cut.add_argument("--distinct", help="Write the k-mers above the count that this fraction of the distinct k-mers stays at or below (default 0.9998).")
    cut.add_argument("--greater_than", help="Write the k-mers with a count above this, in place of --distinct.", type=int)
    kp.add_argument("--forward", help="Count every k-mer as it stands, not under the smaller of itself and its reverse complement.", action='store_true')
    kp.add_argument("--both_strands", help="Write every k-mer's reverse complement behind it.", action='store_true')
    kp.add_argument("--histogram", help="Also write the histogram (count<tab>kmers lines) to this file.")
    kp.add_argument("--chunk_bytes", help="Bytes of the FASTA file per piece.", type=int, default=64 << 20)
    kp.add_argument("--device", help="GPU to use ('cpu': the host backend, one thread).", default="cuda:0")
    gp = sub.add_parser("composition", help="Count a reference's G/C, A/T and soft-masked bases per bin (the table `cnv --composition` takes) from its FASTA file.")
    gp.add_argument("--ref", help="Reference genome, FASTA (a name ending in .gz is inflated on the host).", required=True)
    gp.add_argument("--output", help="Name of the output file (tab-separated, one row per bin).", required=True)
    gp.add_argument("--bin_size", help="Bases per bin: the binned depth's.", type=int, default=1000)
    gp.add_argument("--chunk_bytes", help="Bytes of the FASTA file per piece.", type=int, default=64 << 20)
    gp.add_argument("--device", help="GPU to use ('cpu': the host backend, one thread).", default="cuda:0")
    xp = sub.add_parser("sketch", help="Sketch a reference's window minimizers and write its seed index (the mapper's first stage) from its FASTA file.")
    xp.add_argument("--ref", help="Reference genome, FASTA (a name ending in .gz is inflated on the host).", required=True)
    xp.add_argument("--output", help="Name of the output file (an uncompressed .npz).", required=True)
    xp.add_argument("--weights", help="Repetitive k-mers to down-weight: the output of the kmers mode at the same k (the mapper's -W list).")
    xp.add_argument("--k", help="K-mer size, 1..16.", type=int, default=15)
    xp.add_argument("--w", help="Window size in k-mer positions, 1..256.", type=int, default=50)
    xp.add_argument("--chunk_bytes", help="Bytes of the FASTA file per piece.", type=int, default=64 << 20)
    xp.add_argument("--device", help="GPU to use ('cpu': the host backend, one thread).", default="cuda:0")
    lp = sub.add_parser("filter", help="Write the reads of a FASTQ file that are long and good enough, from one pass over it.")
    lp.add_argument("--fastq", help="FASTQ file of the reads (a name ending in .gz is inflated on the host).", required=True)
    lp.add_argument("--output", help="Name of the FASTQ file of the kept reads.", required=True)
    lp.add_argument("--min_length", help="Drop reads with fewer bases.", type=int, default=0)
    lp.add_argument("--max_length", help="Drop reads with more bases (0: no limit).", type=int, default=0)
    lp.add_argument("--min_mean_quality", help="Drop reads whose mean base quality (the arithmetic mean of the Phred values) is lower.", type=float, default=0.0)
    lp.add_argument("--chunk_bytes", help="Bytes of the FASTQ file per piece.", type=int, default=64 << 20)
    lp.add_argument("--device", help="GPU to use ('cpu': the host backend, one thread).", default="cuda:0")
    for p in (rp, hp, qp, pp, dp, fp, vp, sp, mp, cp):
        add_filter_arguments(p)
    for mode in ("seed", "plot", "cycle2bed"):
        sub.add_parser(mode, help="(reference implementation; not part of the MI355X path)", add_help=False)
    return parser


def reconstruct_mode(args):
    print("Performing reconstruction with options:")
    print_args(args)
    from coral_amd import infer_breakpoint_graph
    b2bn = infer_breakpoint_graph.reconstruct_graph(args)
    if not (args.output_bp or args.skip_cycle_decomp):
        ref = os.environ.get("CORAL_REFERENCE_SRC")
        if ref and ref not in sys.path:
            sys.path.insert(0, ref)
        try:
            import cycle_decomposition            # the reference's module (needs gurobipy)
        except ImportError as e:
            raise SystemExit("cycle decomposition is the reference's Gurobi step and is not available here (%s); "
                             "re-run with --skip_cycle_decomp or --output_bp" % e)
        cycle_decomposition.reconstruct_cycles(args, b2bn)
    b2bn.closebam()
    infer_breakpoint_graph.print_complete_message()
    print("\nCompleted reconstruction.")
    return b2bn


def qc_mode(args):
    """scripts/report_nanopore_qc.py of the reference on the aligned BAM: quality_control_summary.tsv (its lines 70-74), the two
    histograms (lines 54-68, plain matplotlib) and read_qc.json (counters, summary, base-quality histogram)."""
    import json
    from coral_amd import bam
    if (args.lr_bam is None) == (getattr(args, "fastq", None) is None):
        raise SystemExit("qc: give exactly one of --lr_bam and --fastq")
    if args.lr_bam is None:
        if record_filter_of(args).active:
            raise SystemExit("qc: the --filter_* arguments test bam records and cannot be given with --fastq (the filter mode drops reads of a FASTQ file)")
        from coral_amd import fastq
        qc = fastq.read_qc(args.fastq, device=args.device, chunk_bytes=args.chunk_bytes)
    else:
        qc = bam.read_qc(args.lr_bam, device=args.device, record_filter=record_filter_of(args))
    os.makedirs(args.output_dir, exist_ok=True)
    wrote = [qc.write_summary(os.path.join(args.output_dir, "quality_control_summary.tsv"))]
    summary = qc.summary()
    path = os.path.join(args.output_dir, "read_qc.json")
    with open(path, "w") as fp:
        json.dump({"counters": qc.counters, "summary": summary, "base_quality_hist": qc.base_quality_hist.tolist()}, fp, indent=1)
        fp.write("\n")
    wrote.append(path)
    plt = None
    if not args.no_plots:
        try:
            import matplotlib
            matplotlib.use("Agg")
            import matplotlib.pyplot as plt
        except ImportError:
            print("matplotlib is not installed: no histogram images")
    if plt is not None:
        for values, label, title, name in (
                (qc.length, "Mean Sequence Length", "Mean Length of Nanopore Sequences (mean = %s)" % summary["mean_length"], "mean_length_histogram.png"),
                (qc.mean_qualities(), "Mean Sequence Quality", "Mean Quality of Nanopore Sequences (mean = %s)" % summary["mean_quality"],
                 "mean_sequence_quality_histogram.png")):
            plt.figure(figsize=(10, 5))
            plt.hist(values, bins="auto")
            plt.xlabel(label)
            plt.ylabel("Frequency")
            plt.title(title)
            path = os.path.join(args.output_dir, name)
            plt.savefig(path, dpi=300)
            plt.close()
            wrote.append(path)
    for w in wrote:
        print("Wrote %s" % w)
    return wrote


def pileup_mode(args):
    """chrom, pos (0-based), A, C, G, T of every position of the regions whose depth is above 0, in region order."""
    from coral_amd import bam
    if args.bed:
        with open(args.bed) as fp:
            rows = [ln.split() for ln in fp if ln.strip() and not ln.startswith(("#", "track", "browser"))]
        regions = [(r[0], int(r[1]), int(r[2])) for r in rows]
    else:
        regions = []
        for text in args.region:
            chrom, span = text.rsplit(":", 1)
            a, b = span.replace(",", "").split("-")
            regions.append((chrom, int(a), int(b)))
    p = bam.pileup(args.lr_bam, regions, args.min_base_quality, args.read_callback, device=args.device, record_filter=record_filter_of(args))
    with open(args.output, "w") as fp:
        fp.write("chrom\tpos\tA\tC\tG\tT\n")
        for chrom, a, b in p.regions:
            counts = p.counts(chrom, a, b)
            for k in counts.sum(axis=0).nonzero()[0].tolist():
                fp.write("%s\t%d\t%d\t%d\t%d\t%d\n" % ((chrom, a + k) + tuple(counts[:, k].tolist())))
    print("Wrote %s" % args.output)
    return args.output


def depth_mode(args):
    """chromosome, start, end, gene, depth, log2, reads of every bin, in header order (bam.BinnedDepth.write)."""
    from coral_amd import bam
    d = bam.binned_depth(args.lr_bam, args.bin_size, args.min_mapq, args.exclude_flags, not args.no_deletions, device=args.device,
                         record_filter=record_filter_of(args))
    d.write(args.output)
    print("Wrote %s (%d bins)" % (args.output, d.n_bins))
    return args.output


def selection_of(args):
    """(regions, names) of the --region and --names_file arguments; None where there is none."""
    regions = None
    if args.region:
        regions = []
        for text in args.region:
            chrom, span = text.rsplit(":", 1)
            a, b = span.replace(",", "").split("-")
            regions.append((chrom, int(a), int(b)))
    names = None
    if args.names_file:
        with open(args.names_file) as fp:
            names = [ln.strip() for ln in fp if ln.strip()]
    return regions, names


def fastq_mode(args):
    """The selected reads as FASTQ (bam.extract_reads): by regions, by names, both (intersected) or neither (every read)."""
    from coral_amd import bam
    regions, names = selection_of(args)
    if args.stream:
        n, _ = bam.extract_reads(args.lr_bam, regions, names, args.reads_exclude_flags, device="cuda:0" if args.device == "cpu" else args.device,
                                 record_filter=record_filter_of(args), output=args.output)
        print("Wrote %s (%d reads)" % (args.output, n))
        return args.output
    reads = bam.extract_reads(args.lr_bam, regions, names, args.reads_exclude_flags, device=args.device, record_filter=record_filter_of(args))
    reads.write(args.output)
    print("Wrote %s (%d reads)" % (args.output, reads.n))
    return args.output


def write_device_of(args):
    """--gpu_compress: where `view` and `sort` deflate their output (RecordBytes.write's device)."""
    if not args.gpu_compress:
        return "cpu"
    return "cuda:0" if args.device == "cpu" else args.device


def view_mode(args):
    """The selected records as a BAM file (bam.extract_records + RecordBytes.write): the selection of `fastq`, the records
    themselves - alignments, tags and all - under the source's header, with the BAI index on request."""
    from coral_amd import bam
    regions, names = selection_of(args)
    if args.stream:                                              # (bam.view_bam: the same bytes, never whole in host memory)
        if args.level != 1:
            raise ValueError("--stream deflates on the GPU, which has one setting: --level must be 1, got %r" % (args.level,))
        st = bam.view_bam(args.lr_bam, args.output, regions, names, args.reads_exclude_flags, record_filter=record_filter_of(args), index=args.index,
                          device="cuda:0" if args.device == "cpu" else args.device)
        print("Wrote %s (%d records)" % (args.output, st.records))
        return args.output
    rec = bam.extract_records(args.lr_bam, regions, names, args.reads_exclude_flags, device=args.device, record_filter=record_filter_of(args))
    if rec.header is None:                                       # an empty names file: nothing was decoded
        rec.header = bam.bam_header_bytes(args.lr_bam)
    rec.write(args.output, level=args.level, index=args.index, device=write_device_of(args))
    print("Wrote %s (%d records)" % (args.output, rec.n))
    return args.output


def sort_mode(args):
    """The records in coordinate order as a BAM file (bam.sort_bam): `samtools view -bq ... | samtools sort | samtools index`,
    with the --filter_* arguments as the view's tests."""
    from coral_amd import bam
    if args.tmp_dir is not None and not args.stream:
        raise ValueError("--tmp_dir names the spill file's directory: it goes with --stream")
    if args.stream:                                              # (bam.sort_bam_stream: the same bytes, never whole in host memory)
        if args.level != 1:
            raise ValueError("--stream deflates on the GPU, which has one setting: --level must be 1, got %r" % (args.level,))
        st = bam.sort_bam_stream(args.lr_bam, args.output, index=args.index, record_filter=record_filter_of(args), exclude_flags=args.reads_exclude_flags,
                                 device="cuda:0" if args.device == "cpu" else args.device, tmp_dir=args.tmp_dir)
        print("Wrote %s (%d records, %d runs)" % (args.output, st.records, st.runs))
        return args.output
    out = bam.sort_bam(args.lr_bam, args.output, index=args.index, level=args.level, record_filter=record_filter_of(args),
                       exclude_flags=args.reads_exclude_flags, device=args.device, write_device=write_device_of(args))
    print("Wrote %s" % out)
    return out


def import_mode(args):
    """The mapper's SAM text as a BAM file (bam.import_sam): `winnowmap ... | samtools view -bS > x.bam`, line 38 of the
    reference's scripts/align_nanopore_reads.sh, with the --filter_* arguments as a view's tests."""
    from coral_amd import bam
    on_gpu = args.device != "cpu"
    st = bam.import_sam(args.sam, args.output, record_filter=record_filter_of(args), device=args.device, level=1 if on_gpu else args.level,
                        write_device=None if on_gpu or not args.gpu_compress else "cuda:0")
    print("Wrote %s (%d records of %d lines, %d dropped)" % (args.output, st.records, st.lines, st.dropped))
    return args.output


def cnv_mode(args):
    """The .cns of segmented copy number (cnv.segment_depth on the binned depth) and, with --seeds, the seed bed of the reference's
    seed mode (cnv.find_seeds): what scripts/call_cnvs.sh and `CoRAL.py seed` make for `reconstruct`."""
    from coral_amd import bam, cnv
    if not 1 <= args.levels <= 20:
        raise ValueError("--levels must be in 1..20, got %r" % (args.levels,))
    if not 0.0 < args.fdr_q < 1.0:
        raise ValueError("--fdr_q must lie in (0, 1), got %r" % (args.fdr_q,))
    if args.seeds and not args.centromeres:
        raise ValueError("--seeds needs --centromeres: a bed file of the centromeres' p and q rows (none is shipped)")
    if args.seeds and not args.output.endswith(".cns"):
        raise ValueError("--seeds reads --output back as a .cns: its name must end in .cns, got %r" % (args.output,))
    cnv._check_gc_arguments(args.gc_strata, args.gc_min_bins, args.min_called)
    reference = bam.BinnedDepth.read(args.reference_cnn) if args.reference_cnn else None
    if args.depth:
        depth = bam.BinnedDepth.read(args.depth)
    else:
        depth = bam.binned_depth(args.lr_bam, args.bin_size, device=args.device, record_filter=record_filter_of(args))
    comp = None
    if args.composition:
        from coral_amd import composition
        comp = composition.Composition.read(args.composition)
    elif args.ref:
        from coral_amd import composition
        comp = composition.reference_composition(args.ref, depth.bin_size, device=args.device)
    seg = cnv.segment_depth(depth, reference, args.levels, args.fdr_q, device=args.device, composition=comp, gc_strata=args.gc_strata, gc_min_bins=args.gc_min_bins,
                            min_called=args.min_called)
    seg.write(args.output)
    print("Wrote %s (%d segments of %d bins)" % (args.output, len(seg), seg.counts.get("kept", 0)))
    if comp is not None:
        used = seg.gc_bias["stratum_bins"] > 0
        span = seg.gc_bias["bias"][used]
        print("GC correction: %d strata in use, bias %.4f .. %.4f (log2), %d bins masked as uncalled" % (
            int(used.sum()), float(span.min()) if len(span) else 0.0, float(span.max()) if len(span) else 0.0, seg.counts["uncalled"]))
    if args.seeds:
        sizes = args.chrom_sizes if args.chrom_sizes else dict(zip(depth.chroms, depth.lengths))
        seeds = cnv.find_seeds(args.output, args.centromeres, sizes, args.gain, args.min_seed_size, args.max_seg_gap)
        cnv.write_seeds(seeds, args.seeds)
        print("Wrote %s (%d seeds)" % (args.seeds, len(seeds)))
    return args.output


def kmers_mode(args):
    """The repetitive k-mers of --ref (kmers.repetitive_kmers): lines 29-30 of the reference's scripts/align_nanopore_reads.sh, the
    file the mapper takes with -W."""
    from coral_amd import kmers
    kc = kmers.repetitive_kmers(args.ref, args.output, args.k, args.distinct, args.greater_than, canonical=not args.forward, both_strands=args.both_strands,
                                device=args.device, chunk_bytes=args.chunk_bytes)
    print("n_sequences: %d\nn_bases: %d\ntotal: %d\ndistinct: %d\nthreshold: %d" % (kc.n_sequences, kc.n_bases, kc.total, kc.distinct, kc.threshold_used))
    print("Wrote %s (%d lines)" % (args.output, kc.lines_written))
    if args.histogram:
        print("Wrote %s (%d lines)" % (args.histogram, kc.write_histogram(args.histogram)))
    kc.close()
    return args.output


def composition_mode(args):
    """The G/C, A/T and soft-masked bases of --ref per bin (composition.reference_composition): the gc and rmask columns of the
    reference table that the reference's scripts/call_cnvs.sh hands to CNVkit, for `cnv --composition`."""
    from coral_amd import composition
    comp = composition.reference_composition(args.ref, args.bin_size, device=args.device, chunk_bytes=args.chunk_bytes)
    comp.write(args.output)
    print("contigs: %d\npositions: %d\nbins: %d\ngc_fraction: %.6f" % (len(comp.chroms), comp.positions, comp.n_bins, comp.genome_gc()))
    print("Wrote %s (%d rows)" % (args.output, comp.n_bins))
    return args.output


def sketch_mode(args):
    """The minimizer index of --ref (minimizers.write_index): the first stage of the mapper of line 34 of the reference's
    scripts/align_nanopore_reads.sh, with --weights the list its -W takes."""
    from coral_amd import minimizers
    idx = minimizers.write_index(args.ref, args.output, args.k, args.w, args.weights, device=args.device, chunk_bytes=args.chunk_bytes)
    print("contigs: %d\nbases: %d\nminimizers: %d\ndensity: %.6f" % (len(idx.contig_names), idx.positions, idx.n, idx.n / idx.positions if idx.positions else 0.0))
    print("seconds: " + " ".join("%s=%.3f" % (name, minimizers.LAST_SKETCH[name]) for name in ("open", "read", "feed", "upload", "symbols", "sketch", "sort", "write", "wall")))
    print("Wrote %s (%d entries)" % (args.output, idx.n))
    idx.close()
    return args.output


def filter_mode(args):
    """The reads of --fastq that are long and good enough (fastq.read_qc with an output): what the "Quality filter reads" of the
    reference's scripts/report_nanopore_qc.py promises.  The kept records are written exactly as they were read."""
    from coral_amd import fastq
    qc = fastq.read_qc(args.fastq, device=args.device, chunk_bytes=args.chunk_bytes, min_length=args.min_length, max_length=args.max_length,
                       min_mean_quality=args.min_mean_quality, output=args.output)
    print("records: %d\nreads: %d\nbases: %d\nkept_records: %d\nkept_bases: %d" % (qc.n_records, qc.n_reads, qc.total_bases, qc.n_kept, qc.kept_bases))
    print("Wrote %s" % args.output)
    return args.output


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    if argv and argv[0] in ("seed", "plot", "cycle2bed"):
        ref = os.environ.get("CORAL_REFERENCE_SRC")
        if not ref:
            raise SystemExit("mode '%s' is the reference's own code; set CORAL_REFERENCE_SRC to its src/ directory" % argv[0])
        import runpy
        sys.argv = [os.path.join(ref, "CoRAL.py")] + list(argv)
        sys.path.insert(0, ref)
        runpy.run_path(os.path.join(ref, "CoRAL.py"), run_name="__main__")
        return None
    parser = build_parser()
    args = parser.parse_args(argv)
    if args.mode == "reconstruct":
        return reconstruct_mode(args)
    if args.mode == "hsr":
        print("Performing HSR mode with options:")              # CoRAL.py:34-38
        print_args(args)
        from coral_amd import hsr
        return hsr.locate_hsrs(args)
    if args.mode == "index":
        from coral_amd import bam
        out = bam.build_index(args.lr_bam, args.index, device=args.device)
        print("Wrote %s" % out)
        return out
    if args.mode == "qc":
        return qc_mode(args)
    if args.mode == "pileup":
        return pileup_mode(args)
    if args.mode == "depth":
        return depth_mode(args)
    if args.mode == "fastq":
        return fastq_mode(args)
    if args.mode == "view":
        return view_mode(args)
    if args.mode == "sort":
        return sort_mode(args)
    if args.mode == "import":
        return import_mode(args)
    if args.mode == "cnv":
        return cnv_mode(args)
    if args.mode == "kmers":
        return kmers_mode(args)
    if args.mode == "composition":
        return composition_mode(args)
    if args.mode == "sketch":
        return sketch_mode(args)
    if args.mode == "filter":
        return filter_mode(args)
    parser.print_help()
    return None


if __name__ == '__main__':
    main()
