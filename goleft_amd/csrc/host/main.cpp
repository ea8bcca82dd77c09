// goleft-depth: the `depth` entry of the reference's dispatcher
// (/root/reference/cmd/goleft/goleft.go:25-32,:55-69) as a C++ executable.
//   goleft-depth [flags] BAM          or          goleft-depth depth [flags] BAM
//   goleft-depth depthwed -s SIZE a.depth.bed b.depth.bed ...   (the consumer of depth.bed files)
//   goleft-depth multidepth -c CHROM a.bam b.bam ...            (/root/reference/multidepth, its own binary there)
//   goleft-depth covstats [-n N] [-r BED] a.bam b.bam ...       (goleft covstats: coverage and insert-size estimates)
//   goleft-depth indexcov -d DIR [-X X,Y] [-p REGEX] [-n] a.bam b.bam ...   (goleft indexcov: cohort coverage from the .bai indexes)
//   goleft-depth indexsplit -n N [--fai FAI] [-p BED] a.bam b.bam ...       (goleft indexsplit: N regions of about equal data)
//   goleft-depth emdepth [--scales FILE | --normalize [--level L]] [--cnvs FILE] matrix.bed[.gz]   (goleft's emdepth package: copy numbers per site of a depthwed matrix)
//   goleft-depth scales [--level L] matrix.bed[.gz]                         (the factors emdepth --scales takes: dcnv's sample medians carried to one level)
//   goleft-depth debias (--gc-values FILE | --fasta ref.fa) [--window W] matrix.bed[.gz]   (dcnv's ChunkDebiaser: the matrix freed of GC bias; emdepth takes the same as --gc-values | --gc-fasta, --gc-window)
//   goleft-depth cnveval [-m MINOVERLAP] [-s] truth.bed[.gz] test.bed[.gz]   (the reference's cnveval command: precision and recall of a call set, per size class)
//   goleft-depth index [-c] [-m N] [-o OUT] a.bam                            (a .bai as htslib writes it, or a .csi, made on the device: no samtools needed)
//   goleft-depth perbase [-Q Q] [-c CHROM] [-b BED] [--quantize C1,C2,...] [-o OUT] a.bam   (the per-base depth as a bedGraph: runs of equal depth, encoded on the device)
//   goleft-depth dist [-Q Q] [-c CHROM] [-b BED] [--thresholds T1,T2,...] [--max-depth N] --prefix PREFIX a.bam   (the depth distribution, summary and threshold counts, counted on the device)
//   goleft-depth samplename [-e] a.bam                                     (goleft samplename: the @RG SM values)
//   samtools depth -Q q -d D -r REGION in.bam                   (the same program installed under the NAME samtools,
//                                                                goleft_amd/shim/samtools: an unmodified goleft finds it on PATH)
#include <unistd.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../../include/goleft_depth_host.h"

// The outputs are written and closed inside the *_main functions; what is left when they return is giving tens of
// gigabytes of HBM back page by page and unloading the HIP runtime -- work the kernel does for a dying process
// anyway, in a fraction of the time.  A command-line tool leaves at once.
static int leave(int rc)
{
    fflush(stdout);
    fflush(stderr);
    if (getenv("GOLEFT_SLOW_EXIT")) exit(rc);             // a profiler writes its report from an exit handler
    _exit(rc);
}

// the subcommands: the word that selects one, the argv[0] its entry sees, the entry
struct Entry { const char* subcommand; const char* argv0; int (*entry)(int, const char* const*); };
static const Entry kEntries[] = {
    {"depthwed", "goleft depthwed", gdh_depthwed_main}, {"multidepth", "multidepth", gdh_multidepth_main},
    {"covstats", "covstats", gdh_covstats_main},        {"indexcov", "indexcov", gdh_indexcov_main},
    {"indexsplit", "indexsplit", gdh_indexsplit_main},  {"emdepth", "emdepth", gdh_emdepth_main},
    {"scales", "scales", gdh_scales_main},              {"debias", "debias", gdh_debias_main},
    {"samplename", "samplename", gdh_samplename_main},  {"cnveval", "cnveval", gdh_cnveval_main},
    {"index", "index", gdh_index_main},                 {"perbase", "perbase", gdh_perbase_main},
    {"dist", "dist", gdh_dist_main}};

int main(int argc, char** argv)
{
    gdh_set_fast_exit(1);
    std::vector<const char*> av;
    {
        const char* base = strrchr(argv[0], '/');
        base = base ? base + 1 : argv[0];
        if (strcmp(base, "samtools") == 0) {
            for (int i = 0; i < argc; ++i) av.push_back(argv[i]);
            return leave(gdh_samtools_main((int)av.size(), av.data()));
        }
    }
    for (const Entry& e : kEntries)
        if (argc > 1 && strcmp(argv[1], e.subcommand) == 0) {
            av.push_back(e.argv0);
            for (int i = 2; i < argc; ++i) av.push_back(argv[i]);
            return leave(e.entry((int)av.size(), av.data()));
        }
    av.push_back("goleft depth");
    int first = 1;
    if (argc > 1 && strcmp(argv[1], "depth") == 0) first = 2;
    for (int i = first; i < argc; ++i) av.push_back(argv[i]);
    return leave(gdh_depth_main((int)av.size(), av.data()));
}
