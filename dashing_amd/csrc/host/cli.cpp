// cli.cpp -- `dashing-amd`: dashing's `sketch` and `dist` (= `cmp` = `setdist`) subcommands
// (src/main.cpp:22-44) with the two hot loops running on MI355X through the C-ABI
// (include/dashing_hip.h).  Flags keep dashing's spellings (src/dashing.h:35-104,
// src/distmain.cpp:47-100, src/dashing.cpp:253-337): NB -S is log2(sketch bytes) = HLL precision
// and -p is host threads.  HLL sketches only; flags selecting other sketch types / encoders are
// rejected.  There is no CPU compute path: without a gfx950 device the program exits non-zero.
#include <getopt.h>
#include <omp.h>

#include <atomic>
#include <fstream>
#include <limits>
#include <sys/stat.h>
#include <unistd.h>
#include <zlib.h>

#include <algorithm>
#include <cstdarg>
#include <chrono>
#include <functional>
#include <future>
#include <memory>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include <hip/hip_runtime_api.h>  // (--groups: the unions' device buffer)

#include "../../../include/dashing_hip.h"
#include "host.h"

using namespace dshh;

static const char *kVersion = "dashing-amd 0.1 (gfx950; HLL sketch/dist hot path of dashing v1)";

[[noreturn]] static void die(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    std::vfprintf(stderr, fmt, ap);
    va_end(ap);
    std::fputc('\n', stderr);
    std::exit(EXIT_FAILURE);
}

#define DSH(ctx, call)                                                             \
    do {                                                                           \
        int rc_ = (call);                                                          \
        if (rc_) die("[dashing-amd] %s failed (%d): %s", #call, rc_, dsh_last_error(ctx)); \
    } while (0)

static bool isfile(const std::string &p)
{
    struct stat st;
    return ::stat(p.c_str(), &st) == 0 && S_ISREG(st.st_mode);
}

static void usage(const char *sub)
{
    std::fprintf(stderr,
        "%s\nUsage: dashing-amd %s [options] genome1 genome2 ... | -F paths.txt\n"
        "  -k, --kmer-length INT    k (<=32) [31]\n"
        "  -S, --sketch-size INT    log2 sketch size in bytes = HLL precision p [10]\n"
        "  -p, --nthreads INT       host threads for FASTA parsing [1]\n"
        "  -F, --paths FILE         file with one genome path per line\n"
        "  -P, --prefix DIR / -x, --suffix STR   sketch cache location / name suffix\n"
        "  -C, --no-canon           do not canonicalise k-mers\n"
        "  --device INT             GPU ordinal [0]\n"
        "  --ngpus INT | --devices a,b,..  (dist) share the rows of the matrix between several GPUs: -b to a file is written\n"
        "                           by every GPU at its own offsets, other outputs are gathered to the first GPU over RCCL\n", kVersion, sub);
    if (!std::strcmp(sub, "sketch_by_seq") || !std::strcmp(sub, "dist_by_seq"))
        std::fprintf(stderr, "  (by-seq: every sequence RECORD of every input, in input order, is one sketch, labelled by its name -- the\n"
                             "   header up to the first space or tab; sketch_by_seq writes them with -o into this tool's own `sketch -o`\n"
                             "   container + FILE.labels.gz, not upstream's by-seq layout; dist_by_seq --presketched FILE reads that back;\n"
                             "   dist_by_seq refuses -Q, more than one device and -W; DSH_DEVICE_PARSE=1: plain files are parsed on the device)\n");
    if (!std::strcmp(sub, "sketch") || !std::strcmp(sub, "sketch_by_seq")) {
        std::fprintf(stderr, "  -c, --skip-cached        skip genomes whose .hll already exists\n"
                             "  -o FILE                  write all sketches into one file (+ FILE.labels.gz) instead of one .hll per genome\n");
    } else {
        std::fprintf(stderr,
            "  -o, --out-sizes FILE     cardinalities [stdout]\n"
            "  -O, --out-dists FILE     distances [stdout]\n"
            "  -b/-U/-T                 emit binary / PHYLIP upper-triangular / full TSV [upper-triangular TSV]\n"
            "  -M/-l                    Mash distance / full Mash distance [Jaccard index]\n"
            "  -E/-I/-m                 ORIGINAL / ERTL_IMPROVED / ERTL_MLE estimator [ERTL_MLE]\n"
            "  -W, --cache-sketches     read/write <genome>.w.<k>.spacing.<S>.hll next to the input (or in -P)\n"
            "  -H, --presketched        inputs are .hll files\n"
            "  --avoid-sorting          keep input order (default: largest file first)\n"
            "  --threshold FLOAT        emit only the pairs that pass: value >= FLOAT for the similarity measures, <= FLOAT for\n"
            "                           the distances.  Text: '#Threshold<TAB>measure<TAB>op<TAB>FLOAT', then name_i<TAB>name_j<TAB>value\n"
            "                           per hit; -b: u64 n, u64 nnz, u64 row_ptr[n+1], u32 col[nnz], f32 val[nnz]; with -Q one row\n"
            "                           per query.  Not with --nearest-neighbors, -U, -T or several devices.\n"
            "  --cluster FLOAT          emit the single-linkage clusters at FLOAT instead of distances: the connected components of\n"
            "                           the graph whose edges are --threshold FLOAT's pairs, computed on the device.  Text:\n"
            "                           '#Cluster<TAB>measure<TAB>op<TAB>FLOAT', then name<TAB>cluster<TAB>representative per input in\n"
            "                           output order, clusters numbered from 0 by their first member, which represents them;\n"
            "                           -b: u64 n, u64 n_clusters, u32 labels[n] (label = slot of the representative).  Not with\n"
            "                           --threshold, --nearest-neighbors, --pairs, -Q, -U, -T or several devices.\n"
            "  --linkage NAME           with --cluster: single [default: the components above], complete or average -- agglomerate,\n"
            "                           best pair of clusters first, while a pair passes FLOAT under the linkage (worst member\n"
            "                           pair; exact mean of the member pairs in units of 2^-30), on the device (dsh_linkage_threshold).\n"
            "                           With complete or average the '#Cluster' line gains a fifth field, the linkage; -b is the same.\n"
            "                           average not with --sizes.\n"
            "  --min-pts N              with --cluster: density clusters (DBSCAN) instead of the components, on the device\n"
            "                           (dsh_dbscan_threshold).  An input with at least N - 1 others passing FLOAT with it is a core\n"
            "                           (it counts itself); the clusters are the components of the core-core pairs; an input that\n"
            "                           is no core joins the cluster of one core that passes with it (--assign first [default]: the\n"
            "                           first in output order; best: the one with the best value) as a border, else it is noise.\n"
            "                           Text: '#Cluster<TAB>measure<TAB>op<TAB>FLOAT<TAB>dbscan<TAB>N<TAB>first|best', then\n"
            "                           name<TAB>cluster<TAB>representative<TAB>core|border|noise<TAB>degree per input, clusters\n"
            "                           numbered from 0 by their first core, which represents them; noise has '-' for both;\n"
            "                           -b: u64 n, u64 n_clusters, u32 labels[n], u32 degree[n], u8 kind[n] (0 noise, 1 border,\n"
            "                           2 core): no input for --extend or --histogram-labels.  --stats composes.  Not with\n"
            "                           --linkage complete|average.\n"
            "  --representatives FLOAT  emit greedy representatives at FLOAT instead of distances: walk the inputs in output order\n"
            "                           (largest file first by default, the order given with --avoid-sorting); an input that no\n"
            "                           earlier representative passes --threshold FLOAT's test with becomes a representative, every\n"
            "                           other input joins its FIRST such representative.  Computed on the device.  Text:\n"
            "                           '#Representatives<TAB>measure<TAB>op<TAB>FLOAT', then name<TAB>cluster<TAB>representative<TAB>value\n"
            "                           per input, clusters numbered from 0 by ascending representative, value = the pair's value\n"
            "                           ('-' for a representative); -b: u64 n, u64 n_reps, u32 labels[n].  Not with --cluster,\n"
            "                           --threshold, --nearest-neighbors, --pairs, -Q, -U, -T or several devices.\n"
            "  --assign first|best      with --representatives: an input that is no representative joins the FIRST representative\n"
            "                           that passes the test with it [first], or the one with the BEST value (ties: the first).\n"
            "  --extend FILE            with --representatives and --avoid-sorting: FILE is the -b output of an earlier\n"
            "                           --representatives run over the first n_old inputs of this run, in this order; those keep\n"
            "                           their labels and only the inputs behind them are judged, against the old representatives\n"
            "                           and each other.  Outputs keep their formats.\n"
            "  --stats                  with --cluster or --representatives (also with --assign / --extend): the statistics of the\n"
            "                           labelling (dsh_group_stats).  Every text line gains three fields: the name of the group's\n"
            "                           medoid (the member with the best total value to the others), the mean value of the input to\n"
            "                           the other members of its group ('-' where it has none), and the worst such value; -b appends\n"
            "                           u32 medoid[n], u32 cnt[n], i64 sum[n] (values in units of 2^-30), f32 worst[n].  Not with\n"
            "                           --sizes.\n"
            "  --histogram SPEC         emit the distribution of the values instead of the values: how many pairs fall between\n"
            "                           the edges SPEC names, counted on the device in one pass (dsh_dist_histogram).  SPEC is\n"
            "                           lo:hi:nbins (the nbins + 1 edges lo + (hi - lo) * i / nbins), a comma list of numbers, or\n"
            "                           @FILE with one number per line; at most 4096 edges, strictly increasing as float32.  An\n"
            "                           edge is closed on the side that passes --threshold: bins [lo, hi) for the similarity\n"
            "                           measures, (lo, hi] for the distances.  Text: '#Histogram<TAB>measure<TAB>\">=\" or \"<=\"',\n"
            "                           then per class lower<TAB>upper<TAB>count ('-inf' / 'inf' for the outer classes, 'nan' for\n"
            "                           the values that are NaN); -b: u64 n_edges, u64 planes, f32 edges[n_edges] padded to 8\n"
            "                           bytes, u64 counts[planes][n_edges + 2].  With -Q the queries x references rectangle is\n"
            "                           counted, else every pair once (also for the asymmetric measures).  Not with --threshold,\n"
            "                           --cluster, --representatives, --nearest-neighbors, --pairs, -U, -T or several devices.\n"
            "  --histogram-labels FILE  with --histogram: FILE is the -b output of --cluster or --representatives over the same\n"
            "                           inputs in the same order; every line gets two counts, the pairs inside a group and the\n"
            "                           pairs between groups (-b: two planes).\n"
            "  --union-curve            emit how the UNION of the inputs grows as they are added one after the other, in input\n"
            "                           order: the k-mer pangenome growth (collector's) curve, computed on the device from the\n"
            "                           resident sketches (dsh_union_curve).  Text: '#UnionCurve<TAB>estimator<TAB>permutations=N\n"
            "                           <TAB>seed=S', '#step<TAB>name<TAB>union_size<TAB>new[<TAB>perm_mean<TAB>perm_min<TAB>perm_max]',\n"
            "                           then one line per input: its 1-based step, its name, the size of the union up to it and\n"
            "                           what it added (%%.3f).  --curve-permutations N [0]: also the mean, minimum and maximum of\n"
            "                           each step over N random orders (dsh_curve_permutations; --curve-seed S [0]).  -b: u64 n,\n"
            "                           u64 N, f64 curve[1 + N][n]: the given order's curve, then each permutation's.  Not with\n"
            "                           --threshold, --cluster, --representatives, --nearest-neighbors, --histogram, --mst,\n"
            "                           --pairs, --groups, -Q, -U, -T, dist_by_seq or several devices.\n"
            "  --mst                    emit the minimum spanning tree of the pair values instead of the values: the\n"
            "                           single-linkage dendrogram, n - 1 edges that give the --cluster components at EVERY\n"
            "                           threshold (dsh_mst).  Text: '#MST<TAB>measure<TAB>n<TAB>n_edges', then\n"
            "                           name_a<TAB>name_b<TAB>value per edge, best value first (ties: inputs in output order);\n"
            "                           -b: u64 n, u64 n_edges, u32 lhs[n_edges], u32 rhs[n_edges], f32 val[n_edges].\n"
            "                           --mst-cutoff FLOAT: only pairs that pass FLOAT as --threshold would are edges (a forest)\n"
            "                           [every pair whose value is not NaN].  Not with what --cluster refuses, nor with --cluster,\n"
            "                           --representatives, --histogram or --stats.\n"
            "  --dendrogram             with --mst: emit the merge table instead of the edges (dsh_mst_linkage).  Inputs are the\n"
            "                           clusters 0 .. n - 1 in output order, merge s makes cluster n + s.  Text:\n"
            "                           '#Dendrogram<TAB>measure<TAB>n<TAB>n_merges', then a<TAB>b<TAB>value<TAB>size per merge\n"
            "                           (a < b the cluster ids); -b: u64 n, u64 n_merges, u32 a[], u32 b[], f32 value[], u32 size[].\n"
            "  --pairs FILE             emit only the pairs FILE lists, one per line as name_a<TAB>name_b (input names as given\n"
            "                           here; record names with dist_by_seq), in FILE's order: name_a<TAB>name_b and one value per\n"
            "                           measure.  --measures LIST: comma-separated from MASH_DIST, JI, SIZES, FULL_MASH_DIST,\n"
            "                           FULL_CONTAINMENT_DIST, CONTAINMENT_INDEX, CONTAINMENT_DIST, SYMMETRIC_CONTAINMENT_INDEX,\n"
            "                           SYMMETRIC_CONTAINMENT_DIST [the measure the other flags select].  Not with -Q,\n"
            "                           --nearest-neighbors, --threshold, -b or several devices.\n"
            "  --groups FILE            compare the UNIONS of groups of inputs instead of the inputs: FILE lists name<TAB>group per\n"
            "                           line, every input exactly once; the groups, in order of first appearance, take the\n"
            "                           inputs' place in every output (labels, -o sizes, all formats, --threshold,\n"
            "                           --nearest-neighbors).  Not with --pairs, -Q, dist_by_seq or several devices.\n"
            "  --presketched            .hll files sketched at a HIGHER precision than -S are folded to -S as they are loaded\n");
    }
    std::exit(EXIT_FAILURE);
}

struct Opts {
    int k = 31, S = 10, nthreads = 1, canon = 1, device = 0;
    int estim = ERTL_MLE, result_type = JI, fmt = UT_TSV;
    int cache = 0, presketched = 0, avoid_sorting = 0, skip_cached = 0;
    unsigned nneighbors = 0;  // --nearest-neighbors
    bool has_threshold = false;  // --threshold: only the pairs that pass, as (name, name, value) lines or CSR (-b)
    float threshold = 0.f;
    int linkage = -1;          // --linkage: -1 not given, else DSH_LINKAGE_* (complete / average: dsh_linkage_threshold)
    bool has_cluster = false;  // --cluster: the connected components of --threshold's graph (dsh_cluster_threshold)
    float cluster_t = 0.f;
    bool has_min_pts = false;  // --min-pts N with --cluster: density clusters (dsh_dbscan_threshold)
    uint32_t min_pts = 0;
    bool has_reps = false;  // --representatives: the greedy pass in output order over --threshold's graph (dsh_greedy_threshold)
    float reps_t = 0.f;
    int assign_mode = DSH_GREEDY_FIRST;  // --assign first|best (dsh_greedy_extend)
    bool has_assign = false;
    bool has_stats = false;  // --stats: medoid, mean and worst value per input of the labelling (dsh_group_stats)
    bool has_mst = false;  // --mst [--mst-cutoff FLOAT] [--dendrogram]: the minimum spanning tree of the pair values (dsh_mst)
    bool has_mst_cutoff = false, dendrogram = false;
    float mst_cutoff = 0.f;
    bool has_hist = false;  // --histogram SPEC: the distribution of the values over the edges of SPEC (dsh_dist_histogram)
    std::vector<float> hist_edges;
    std::string hist_labels_file;  // --histogram-labels FILE: counts split into intra-group and inter-group pairs
    bool has_curve = false;  // --union-curve [--curve-permutations N] [--curve-seed S]: the growth of the union in input order (dsh_union_curve)
    bool has_curve_perms = false, has_curve_seed = false;
    uint64_t curve_perms = 0, curve_seed = 0;
    std::string extend_file;  // --extend FILE: the labels of an earlier --representatives -b run over the first inputs
    std::string groups_file;  // --groups FILE: the unions of named groups are compared instead of the inputs (dsh_union_groups)
    std::string pairs_file, measures;  // --pairs FILE [--measures LIST]: only the listed pairs (dsh_dist_pairs)
    int rccl = 0;             // --rccl: deliver the rows through the RCCL exchange of the C-ABI even with one device
    std::vector<int> devices;  // --devices a,b,... / --ngpus G: GPUs sharing the all-pairs rows (binary output)
    std::string paths_file, prefix, suffix, spacing, out_sizes, out_dists;
    std::vector<std::string> inpaths, querypaths;
};

// --stats: what dsh_group_stats says about the labels of --cluster / --representatives, and its two output forms
struct GroupStats {
    std::vector<uint32_t> medoid, cnt;
    std::vector<int64_t> sum;
    std::vector<float> worst;
    void compute(dsh_ctx *ctx, const Opts &o, const std::vector<uint32_t> &labels, size_t n)
    {
        medoid.resize(std::max<size_t>(n, 1)), cnt.resize(std::max<size_t>(n, 1)), sum.resize(std::max<size_t>(n, 1)), worst.resize(std::max<size_t>(n, 1));
        DSH(ctx, dsh_group_stats(ctx, o.estim, o.result_type, o.k, labels.data(), medoid.data(), cnt.data(), sum.data(), worst.data()));
    }
    // behind labels[n]: u32 medoid[n], u32 cnt[n], i64 sum[n], f32 worst[n]
    void write_binary(std::FILE *fp, size_t n) const
    {
        if (std::fwrite(medoid.data(), sizeof(uint32_t), n, fp) != n || std::fwrite(cnt.data(), sizeof(uint32_t), n, fp) != n ||
            std::fwrite(sum.data(), sizeof(int64_t), n, fp) != n || std::fwrite(worst.data(), sizeof(float), n, fp) != n)
            die("Error writing to binary file");
    }
    // <TAB>medoid's name<TAB>mean value to the own group ('-': no pair)<TAB>worst value, in --threshold's number format
    void append_fields(std::string &s, size_t x, const std::vector<std::string> &names) const
    {
        char num[64];
        s += '\t';
        s += names[medoid[x]];
        if (!cnt[x]) s += "\t-";
        else s.append(num, (size_t)std::snprintf(num, sizeof num, "\t%.6g", (double)sum[x] / (double)cnt[x] / (double)(1ll << DSH_STATS_FRAC_BITS)));
        s.append(num, (size_t)std::snprintf(num, sizeof num, "\t%.6g", (double)worst[x]));
    }
};

// one number of a --histogram SPEC (strtod's syntax: inf and -inf included), whole token; NaN is no edge
static double histogram_number(const std::string &tok, const char *spec)
{
    char *end = nullptr;
    const double v = std::strtod(tok.c_str(), &end);
    if (tok.empty() || end == tok.c_str() || *end || v != v) die("--histogram: '%s' in '%s' is not a number", tok.c_str(), spec);
    return v;
}

// --histogram SPEC: lo:hi:nbins | a comma list of numbers | @FILE with one number per line -> the float32 edges
static std::vector<float> parse_histogram_spec(const char *spec)
{
    const std::string sp(spec);
    std::vector<float> e;
    if (!sp.empty() && sp[0] == '@') {
        std::ifstream f(sp.substr(1));
        if (!f) die("--histogram: could not open %s", sp.c_str() + 1);
        std::string line;
        while (std::getline(f, line)) {
            while (!line.empty() && (line.back() == '\r' || line.back() == ' ' || line.back() == '\t')) line.pop_back();
            if (line.empty()) continue;
            e.push_back((float)histogram_number(line, spec));
        }
    } else if (sp.find(':') != std::string::npos) {
        const size_t c1 = sp.find(':'), c2 = sp.find(':', c1 + 1);
        if (c2 == std::string::npos || sp.find(':', c2 + 1) != std::string::npos) die("--histogram: '%s' is not lo:hi:nbins", spec);
        const double lo = histogram_number(sp.substr(0, c1), spec), hi = histogram_number(sp.substr(c1 + 1, c2 - c1 - 1), spec);
        const std::string nb = sp.substr(c2 + 1);
        char *end = nullptr;
        const long nbins = std::strtol(nb.c_str(), &end, 10);
        if (nb.empty() || *end || nbins < 1 || nbins + 1 > DSH_HIST_MAX_EDGES)
            die("--histogram: '%s' needs between 1 and %d bins", spec, DSH_HIST_MAX_EDGES - 1);
        if (!(lo < hi) || lo - lo != 0 || hi - hi != 0) die("--histogram: '%s' needs finite lo < hi", spec);
        for (long i = 0; i <= nbins; ++i) e.push_back((float)(lo + (hi - lo) * (double)i / (double)nbins));
    } else {
        for (size_t b = 0; b <= sp.size();) {
            const size_t c = std::min(sp.find(',', b), sp.size());
            e.push_back((float)histogram_number(sp.substr(b, c - b), spec));
            b = c + 1;
        }
    }
    if (e.empty() || e.size() > (size_t)DSH_HIST_MAX_EDGES) die("--histogram: '%s' gives %zu edges: between 1 and %d", spec, e.size(), DSH_HIST_MAX_EDGES);
    for (size_t b = 1; b < e.size(); ++b)
        if (!(e[b - 1] < e[b]))
            die("--histogram: '%s': edge %zu (%.9g) is not above edge %zu (%.9g) as float32: the edges must increase strictly", spec, b,
                (double)e[b], b - 1, (double)e[b - 1]);
    return e;
}

// the labels of a --cluster -b / --representatives -b file: u64 n, u64 count, u32 labels[n] (what --extend and
// --histogram-labels read)
static std::vector<uint32_t> read_labels_binary(const char *flag, const std::string &path)
{
    std::FILE *ef = std::fopen(path.c_str(), "rb");
    if (!ef) die("%s: could not open %s", flag, path.c_str());
    uint64_t hdr[2] = {0, 0};
    if (std::fread(hdr, sizeof(uint64_t), 2, ef) != 2) die("%s: %s is too short for the header of a --cluster -b or --representatives -b file", flag, path.c_str());
    if (std::fseek(ef, 0, SEEK_END) != 0) die("%s: could not read %s", flag, path.c_str());
    const long fsize = std::ftell(ef);
    if (hdr[0] > 0xFFFFFFFFull || fsize < 0 || (uint64_t)fsize != 16 + 4 * hdr[0])
        die("%s: %s has the wrong length for the %llu labels its header announces", flag, path.c_str(), (unsigned long long)hdr[0]);
    std::vector<uint32_t> labels((size_t)hdr[0]);
    if (std::fseek(ef, 16, SEEK_SET) != 0 || std::fread(labels.data(), sizeof(uint32_t), labels.size(), ef) != labels.size())
        die("%s: could not read %s", flag, path.c_str());
    std::fclose(ef);
    return labels;
}

// the FLOAT of --threshold / --cluster / --representatives: a whole token, no NaN
static float float_option(const char *flag, const char *arg)
{
    char *end = nullptr;
    const float v = std::strtof(arg, &end);
    if (end == arg || *end || v != v) die("%s needs a number, got '%s'", flag, arg);
    return v;
}

enum { OPT_PRESKETCHED = 1000, OPT_AVOID_SORT, OPT_DEVICE, OPT_NPERBATCH, OPT_NN, OPT_NGPUS, OPT_DEVICES, OPT_RCCL, OPT_THRESHOLD, OPT_CLUSTER, OPT_LINKAGE, OPT_MIN_PTS, OPT_REPS, OPT_ASSIGN, OPT_EXTEND, OPT_STATS, OPT_HISTOGRAM, OPT_HISTOGRAM_LABELS, OPT_UNION_CURVE, OPT_CURVE_PERMS, OPT_CURVE_SEED, OPT_MST, OPT_MST_CUTOFF, OPT_DENDROGRAM, OPT_PAIRS, OPT_MEASURES, OPT_GROUPS, OPT_UNSUPPORTED };

static Opts parse(int argc, char **argv, bool is_dist)
{
    Opts o;
    static const option longopts[] = {
        {"kmer-length", required_argument, nullptr, 'k'}, {"sketch-size", required_argument, nullptr, 'S'},
        {"nthreads", required_argument, nullptr, 'p'}, {"paths", required_argument, nullptr, 'F'},
        {"prefix", required_argument, nullptr, 'P'}, {"suffix", required_argument, nullptr, 'x'},
        {"no-canon", no_argument, nullptr, 'C'}, {"out-sizes", required_argument, nullptr, 'o'},
        {"out-dists", required_argument, nullptr, 'O'}, {"emit-binary", no_argument, nullptr, 'b'},
        {"phylip", no_argument, nullptr, 'U'}, {"full-tsv", no_argument, nullptr, 'T'},
        {"mash-dist", no_argument, nullptr, 'M'}, {"full-mash-dist", no_argument, nullptr, 'l'},
        // dashing declares these long forms with required_argument (LO_ARG, src/dashing.h:62-64);
        // that is a quirk, scripts use the short forms.  We take them without an argument.
        {"original", no_argument, nullptr, 'E'}, {"improved", no_argument, nullptr, 'I'},
        {"ertl-mle", no_argument, nullptr, 'm'}, {"cache-sketches", no_argument, nullptr, 'W'},
        {"presketched", no_argument, nullptr, OPT_PRESKETCHED}, {"avoid-sorting", no_argument, nullptr, OPT_AVOID_SORT},
        {"skip-cached", no_argument, nullptr, 'c'}, {"device", required_argument, nullptr, OPT_DEVICE},
        {"ngpus", required_argument, nullptr, OPT_NGPUS}, {"devices", required_argument, nullptr, OPT_DEVICES},
        {"rccl", no_argument, nullptr, OPT_RCCL},
        {"nperbatch", required_argument, nullptr, OPT_NPERBATCH}, {"spacing", required_argument, nullptr, 's'},
        {"window-size", required_argument, nullptr, 'w'}, {"help", no_argument, nullptr, 'h'},
        {"use-bb-minhash", no_argument, nullptr, OPT_UNSUPPORTED}, {"use-range-minhash", no_argument, nullptr, OPT_UNSUPPORTED},
        {"use-bloom-filter", no_argument, nullptr, OPT_UNSUPPORTED}, {"use-nthash", no_argument, nullptr, OPT_UNSUPPORTED},
        {"use-cyclic-hash", no_argument, nullptr, OPT_UNSUPPORTED}, {"countmin", no_argument, nullptr, OPT_UNSUPPORTED},
        {"nearest-neighbors", required_argument, nullptr, OPT_NN}, {"threshold", required_argument, nullptr, OPT_THRESHOLD},
        {"cluster", required_argument, nullptr, OPT_CLUSTER}, {"linkage", required_argument, nullptr, OPT_LINKAGE}, {"min-pts", required_argument, nullptr, OPT_MIN_PTS}, {"representatives", required_argument, nullptr, OPT_REPS},
        {"assign", required_argument, nullptr, OPT_ASSIGN}, {"extend", required_argument, nullptr, OPT_EXTEND},
        {"stats", no_argument, nullptr, OPT_STATS},
        {"histogram", required_argument, nullptr, OPT_HISTOGRAM}, {"histogram-labels", required_argument, nullptr, OPT_HISTOGRAM_LABELS},
        {"union-curve", no_argument, nullptr, OPT_UNION_CURVE}, {"curve-permutations", required_argument, nullptr, OPT_CURVE_PERMS},
        {"curve-seed", required_argument, nullptr, OPT_CURVE_SEED},
        {"mst", no_argument, nullptr, OPT_MST}, {"mst-cutoff", required_argument, nullptr, OPT_MST_CUTOFF}, {"dendrogram", no_argument, nullptr, OPT_DENDROGRAM},
        {"pairs", required_argument, nullptr, OPT_PAIRS}, {"groups", required_argument, nullptr, OPT_GROUPS}, {"measures", required_argument, nullptr, OPT_MEASURES},
        // second arm of result_cmp (src/dashing.h:577-588); flag numbers as in DIST_LONG_OPTS
        {"sizes", no_argument, nullptr, 'Z'}, {"containment-index", no_argument, nullptr, 131},
        {"containment-dist", no_argument, nullptr, 132}, {"full-containment-dist", no_argument, nullptr, 133},
        {"symmetric-containment-index", no_argument, nullptr, 137}, {"symmetric-containment-dist", no_argument, nullptr, 138},
        {"query-paths", required_argument, nullptr, 'Q'},
        {nullptr, 0, nullptr, 0}};
    int co;
    optind = 1;
    while ((co = getopt_long(argc, argv, "k:S:p:F:P:x:Co:O:bUTMlEImWHcs:w:eh?8yJQ:Z", longopts, nullptr)) >= 0) {
        switch (co) {
        case 'k': o.k = std::atoi(optarg); break;
        case 'S': o.S = std::atoi(optarg); break;
        case 'p': o.nthreads = std::max(1, std::atoi(optarg)); break;
        case 'F': o.paths_file = optarg; break;
        case 'P': o.prefix = optarg; break;
        case 'x': o.suffix = optarg; break;
        case 'C': o.canon = 0; break;
        case 'o': o.out_sizes = optarg; break;
        case 'O': o.out_dists = optarg; break;
        case 'b': o.fmt = BINARY; break;
        case 'U': o.fmt = UPPER_TRIANGULAR; break;
        case 'T': o.fmt = FULL_TSV; break;
        case 'M': o.result_type = MASH_DIST; break;
        case 'l': o.result_type = FULL_MASH_DIST; break;
        case 'E': o.estim = ORIGINAL; break;
        case 'I': o.estim = ERTL_IMPROVED; break;
        case 'm': o.estim = ERTL_MLE; break;
        case 'W': o.cache = 1; break;
        case 'H': case OPT_PRESKETCHED: o.presketched = 1; break;  // dashing ignores short -H; we honour it
        case OPT_AVOID_SORT: o.avoid_sorting = 1; break;
        case 'c': o.skip_cached = 1; break;
        case OPT_DEVICE: o.device = std::atoi(optarg); break;
        case OPT_NGPUS: {
            const int g = std::atoi(optarg);
            if (g < 1) die("--ngpus needs a positive count");
            o.devices.clear();
            for (int d = 0; d < g; ++d) o.devices.push_back(o.device + d);
            break;
        }
        case OPT_DEVICES: {  // explicit list; a device may repeat (used to test the sharding on one GPU)
            o.devices.clear();
            for (const char *q = optarg; *q;) {
                o.devices.push_back(std::atoi(q));
                while (*q && *q != ',') ++q;
                if (*q == ',') ++q;
            }
            break;
        }
        case OPT_RCCL: o.rccl = 1; break;
        case OPT_NPERBATCH: case 'e': break;  // accepted, no effect here
        case 's': if (optarg && *optarg) die("spaced seeds are out of scope (HLL hot path only)"); break;
        case 'w': if (std::atoi(optarg) > 0) die("minimizer windows are out of scope (HLL hot path only)"); break;
        case 'Z': o.result_type = 2; break;
        case 131: o.result_type = 5; break;
        case 132: o.result_type = 6; break;
        case 133: o.result_type = 4; break;
        case 137: o.result_type = 7; break;
        case 138: o.result_type = 8; break;
        case 'Q': o.querypaths = read_paths_file(optarg); break;
        case OPT_NN:
            if (std::atoi(optarg) <= 0) die("--nearest-neighbors needs a positive count");
            o.nneighbors = (unsigned)std::atoi(optarg);
            break;
        case OPT_THRESHOLD: o.threshold = float_option("--threshold", optarg), o.has_threshold = true; break;
        case OPT_CLUSTER: o.cluster_t = float_option("--cluster", optarg), o.has_cluster = true; break;
        case OPT_LINKAGE:
            o.linkage = !std::strcmp(optarg, "single") ? DSH_LINKAGE_SINGLE : !std::strcmp(optarg, "complete") ? DSH_LINKAGE_COMPLETE
                        : !std::strcmp(optarg, "average") ? DSH_LINKAGE_AVERAGE : -1;
            if (o.linkage < 0) die("--linkage takes single, complete or average, not '%s'.", optarg);
            break;
        case OPT_MIN_PTS: {
            char *end = nullptr;
            const unsigned long long v = std::strtoull(optarg, &end, 10);
            if (end == optarg || *end || *optarg == '-' || v < 1 || v > 0xFFFFFFFFull) die("--min-pts needs a count of at least 1, got '%s'", optarg);
            o.min_pts = (uint32_t)v, o.has_min_pts = true;
            break;
        }
        case OPT_REPS: o.reps_t = float_option("--representatives", optarg), o.has_reps = true; break;
        case OPT_ASSIGN:
            if (!std::strcmp(optarg, "first")) o.assign_mode = DSH_GREEDY_FIRST;
            else if (!std::strcmp(optarg, "best")) o.assign_mode = DSH_GREEDY_BEST;
            else die("--assign takes 'first' or 'best', got '%s'", optarg);
            o.has_assign = true;
            break;
        case OPT_EXTEND: o.extend_file = optarg; break;
        case OPT_STATS: o.has_stats = true; break;
        case OPT_MST: o.has_mst = true; break;
        case OPT_MST_CUTOFF: o.mst_cutoff = float_option("--mst-cutoff", optarg), o.has_mst_cutoff = true; break;
        case OPT_DENDROGRAM: o.dendrogram = true; break;
        case OPT_HISTOGRAM:
            o.hist_edges = parse_histogram_spec(optarg);
            o.has_hist = true;
            break;
        case OPT_HISTOGRAM_LABELS: o.hist_labels_file = optarg; break;
        case OPT_UNION_CURVE: o.has_curve = true; break;
        case OPT_CURVE_PERMS: case OPT_CURVE_SEED: {
            const char *name = co == OPT_CURVE_PERMS ? "--curve-permutations" : "--curve-seed";
            char *end = nullptr;
            const unsigned long long v = std::strtoull(optarg, &end, 10);
            if (end == optarg || *end || *optarg == '-' || (co == OPT_CURVE_PERMS && v > 0xFFFFFFFFull)) die("%s needs a count of at least 0, got '%s'", name, optarg);
            if (co == OPT_CURVE_PERMS) o.curve_perms = v, o.has_curve_perms = true;
            else o.curve_seed = v, o.has_curve_seed = true;
            break;
        }
        case OPT_PAIRS: o.pairs_file = optarg; break;
        case OPT_MEASURES: o.measures = optarg; break;
        case OPT_GROUPS: o.groups_file = optarg; break;
        case '8': case 'y': case 'J': case OPT_UNSUPPORTED:
            die("this option selects a sketch type / emitter outside the HLL sketch+dist hot path");
        default: usage(is_dist ? "dist" : "sketch");
        }
    }
    if (o.k < 1 || o.k > 32) die("k must be in [1,32] for 2-bit encoded k-mers (src/distmain.cpp:101)");
    if (o.S < 4 || o.S > 17) die("-S (log2 sketch bytes) must be in [4,17]");
    o.inpaths = o.paths_file.empty() ? std::vector<std::string>(argv + optind, argv + argc) : read_paths_file(o.paths_file);
    if (o.inpaths.empty()) {
        std::fprintf(stderr, "No paths. See usage.\n");
        usage(is_dist ? "dist" : "sketch");
    }
    return o;
}

static double now_s()
{
    return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
static const bool g_timing = std::getenv("DSH_TIMING") != nullptr;  // phase times on stderr
// (DSH_TIMING with DSH_T0 = the launcher's wall clock in seconds since the epoch: where the process is, seen from outside)
static void since_launch(const char *what)
{
    const char *t0 = std::getenv("DSH_T0");
    if (!g_timing || !t0) return;
    const double now = std::chrono::duration<double>(std::chrono::system_clock::now().time_since_epoch()).count();
    std::fprintf(stderr, "[timing] %s: %.3f s after the launch\n", what, now - std::atof(t0));
}

// File bytes per sketching batch, and the page-locked staging buffers the batches cycle through.  The batches of a large
// input travel back to back: batch b is parsed (or, for plain FASTA, just read: the device decodes it) into buffer b % 3
// and enqueued at once -- host-to-device copy + kernels behind the previous batch on the context's stream -- while the
// host already fills the next buffer; a buffer is only waited for when its turn comes again (a ticket per batch).
// Round 5 waited for batch b - 1 before enqueueing batch b (two buffers): 4.9 ms per 128 MB = 27 GB/s where the copy
// alone takes 2.6 ms (profiles/rd6c/cli_e2e_timing.jsonl).
static const size_t kSketchBatchBytes = (size_t)48 << 20;
constexpr int kStageBufs = 3;
// plain FASTA is decoded on the device (dsh_sketch_fastx_batch_async: the host only read()s the file bytes into the
// staging); DSH_HOST_PARSE=1 keeps the host parser for everything (A/B, and the path compressed inputs and pipes take anyway)
static const bool g_device_parse = std::getenv("DSH_HOST_PARSE") == nullptr;

// page-locked staging is only worth allocating (pinning runs at ~3 GB/s) when the input does not fit one batch: the
// first batch is parsed into pageable memory anyway
static size_t staging_bytes_for(const std::vector<std::string> &paths)
{
    uint64_t total = 0;
    for (const auto &p : paths) {
        total += genome_file_size(p);
        if (total > kSketchBatchBytes) return kSketchBatchBytes + (kSketchBatchBytes >> 3);
    }
    return 0;
}

// The GPU context is created on its own thread while the host already parses the first batch: bringing the HIP
// runtime up costs ~0.1-0.2 s, as much as reading gigabases of FASTA on 16 threads.  The same thread then page-locks the
// staging buffers ONE BY ONE (stage_ready counts them): the main thread takes each as soon as it exists.
struct CtxFuture {
    std::promise<dsh_ctx *> ready;
    std::future<dsh_ctx *> fut;
    std::future<void> done;  // the context thread itself
    dsh_ctx *ctx = nullptr;
    uint8_t *stage[kStageBufs] = {};  // page-locked staging for fill_sketches, allocated on the ctx thread too
    std::atomic<int> stage_ready{0};
    size_t stage_cap = 0;
    CtxFuture(int device, size_t n, int S, size_t staging_bytes = 0)
    {
        fut = ready.get_future();
        stage_cap = staging_bytes;
        done = std::async(std::launch::async, [this, device, n, S, staging_bytes]() {
            const double t0 = now_s();
            dsh_ctx *c = nullptr;
            if (int rc = dsh_create(device, &c)) die("[dashing-amd] no usable gfx950 device (dsh_create = %d); there is no CPU fallback", rc);
            DSH(c, dsh_sketches_alloc(c, n, S));
            (void)dsh_preload(device, DSH_PRELOAD_SKETCH);  // (the main thread is still staging its first batch)
            ready.set_value(c);  // the main thread may use the context from here on
            const double t1 = now_s();
            if (staging_bytes) {
                for (int b = 0; b < kStageBufs; ++b) {
                    if (!(stage[b] = (uint8_t *)dsh_alloc_host(staging_bytes))) die("could not allocate %zu bytes of pinned host memory", staging_bytes);
                    stage_ready.store(b + 1, std::memory_order_release);
                }
            }
            (void)dsh_preload(device, DSH_PRELOAD_COMPARE);  // (beside the main thread's sketching: dist finds its kernels loaded)
            if (g_timing) std::fprintf(stderr, "[timing] on the context thread: dsh_create + alloc %.3f s, pinned staging %.3f s\n", t1 - t0, now_s() - t1);
        });
    }
    dsh_ctx *get()
    {
        if (!ctx) ctx = fut.get();
        return ctx;
    }
    // staging buffer b, once the context thread has page-locked it (nullptr: none were asked for)
    uint8_t *take_stage(int b)
    {
        if (!stage_cap) return nullptr;
        while (stage_ready.load(std::memory_order_acquire) <= b) std::this_thread::sleep_for(std::chrono::microseconds(100));
        uint8_t *p = stage[b];
        stage[b] = nullptr;
        return p;
    }
    ~CtxFuture()
    {
        if (done.valid()) done.get();
        for (auto &b : stage)
            if (b) dsh_free_host(b);
    }
};

// Hot loop 1 (src/sketch_and_cmp.h:314-360, 484-528) as a stream: genomes are taken in batches of <= ~48 MB of
// file bytes; a batch is staged by the host threads STRAIGHT INTO page-locked memory (every genome has its region
// reserved from the file sizes) -- the raw bytes of plain FASTA files, which the device decodes
// (dsh_sketch_fastx_batch_async), or the sequence the host parser extracts (compressed inputs, pipes, multi-line FASTQ; what is
// left of the region filled with 'N') -- and enqueued at once; the staging buffers take turns (see kStageBufs).  Cache
// hits (-W / sketch -c) read the .hll instead; .hll files of a batch are written when its buffer's turn comes again.
static void fill_sketches(CtxFuture &cf, const Opts &o, bool write_files, bool skip_cached, bool load_cached = false)
{
    const size_t n = o.inpaths.size();
    const size_t m = (size_t)1 << o.S;
    const size_t batch_bytes = kSketchBatchBytes;
    // staging: the FIRST batch goes to pageable memory (the HIP runtime is still coming up on the context thread, and
    // page-locking memory needs it); later batches cycle through the page-locked buffers that thread allocates meanwhile
    uint8_t *pin[kStageBufs] = {};
    size_t pin_cap[kStageBufs] = {};
    bool pin_taken[kStageBufs] = {};
    std::unique_ptr<uint8_t[]> first_stage;  // uninitialised: the parsing threads touch its pages first
    struct Flight {  // a batch whose copy + kernels are enqueued: what is left to do on the host when its buffer is reused
        bool valid = false;
        uint64_t ticket = 0;
        std::vector<size_t> slots;       // staged genome t -> its slot (= index into o.inpaths)
        std::vector<std::string> fnames;
        std::vector<char> raw;           // decoded on the device: its status word says whether the device took it
    } fl[kStageBufs];
    uint32_t *status[kStageBufs] = {};   // per buffer: the device decoder's verdict per staged genome (page-locked)
    size_t status_cap[kStageBufs] = {};
    auto sketch_on_host = [&](dsh_ctx *ctx, size_t slot) {  // a genome the staged path could not take: parsed growably, sketched on its own
        std::vector<uint8_t> whole;
        for (const auto &f2 : split_genome_paths(o.inpaths[slot])) {
            if (!whole.empty()) whole.push_back('N');
            if (append_fastx(f2, whole) < 0) die("Could not open %s", f2.c_str());
        }
        whole.push_back('N');
        const uint64_t loff[2] = {0, whole.size()};
        DSH(ctx, dsh_sketch_batch(ctx, whole.data(), loff, 1, slot, o.k, o.canon, nullptr));  // (max-merged into its slot)
    };
    auto retire = [&](int x) {  // the batch that last used buffer x has been sketched: refusals, .hll files
        Flight &f = fl[x];
        if (!f.valid) return;
        dsh_ctx *ctx = cf.get();
        DSH(ctx, dsh_event_wait(ctx, f.ticket));
        for (size_t t = 0; t < f.slots.size(); ++t)
            if (f.raw[t] && status[x][t]) sketch_on_host(ctx, f.slots[t]);  // not what its first byte promised (a '+' line in FASTA, multi-line FASTQ ...)
        if (write_files && !f.slots.empty()) {
            std::vector<uint8_t> rows(f.slots.size() * m);
            size_t r0 = 0;
            while (r0 < f.slots.size()) {  // consecutive slots in one download
                size_t r1 = r0 + 1;
                while (r1 < f.slots.size() && f.slots[r1] == f.slots[r1 - 1] + 1) ++r1;
                DSH(ctx, dsh_download_sketches(ctx, f.slots[r0], r1 - r0, rows.data() + r0 * m));
                r0 = r1;
            }
#pragma omp parallel for schedule(dynamic) num_threads(o.nthreads)
            for (long t = 0; t < (long)f.slots.size(); ++t)
                if (write_hll(f.fnames[t], rows.data() + (size_t)t * m, o.S, o.estim, o.estim, false, 0.0)) die("Could not write %s", f.fnames[t].c_str());
        }
        f.valid = false;
    };
    size_t g = 0, bi = 0;
    while (g < n) {
        const double t_b0 = now_s();
        const int x = (int)(bi % kStageBufs);
        retire(x);
        // the batch: genomes [g, e) whose files total <= batch_bytes (at least one)
        // (the FIRST batch is small: it travels from pageable memory, a synchronous staged copy, while the page-locked buffers
        // are still being allocated)
        const size_t limit = (bi == 0 && cf.stage_cap) ? std::min<size_t>(batch_bytes, (size_t)8 << 20) : batch_bytes;  // (an input of one batch stays one)
        size_t e = g, bytes = 0;
        while (e < n && (e == g || bytes + genome_file_size(o.inpaths[e]) <= limit)) bytes += genome_file_size(o.inpaths[e++]);
        const size_t nb = e - g;
        std::vector<int> cached(nb, 0), gz(nb, 0);
        std::vector<int> rawkind(nb, 0);        // plain FASTA whose raw bytes are staged: decoded on the device
        std::vector<uint64_t> rawlen_of(nb, 0);
        std::vector<std::string> fnames(nb);
        std::vector<std::vector<std::string>> files(nb);
        std::vector<std::vector<uint8_t>> zseq(nb);  // genomes whose sequence length the file size does not bound: compressed
                                                     // files, FIFOs, /dev/stdin, process substitutions (parsed growably)
        std::vector<size_t> late;  // slots of plain files that outgrew their region: sketched on their own after the batch
#pragma omp parallel for schedule(dynamic) num_threads(o.nthreads)
        for (long i = 0; i < (long)nb; ++i) {
            const std::string &entry = o.inpaths[g + i];
            fnames[i] = make_fname(entry, (unsigned)o.S, o.k, o.spacing, o.suffix, o.prefix);
            if ((o.cache || skip_cached) && isfile(fnames[i])) {
                cached[i] = 1;
                continue;
            }
            files[i] = split_genome_paths(entry);
            for (const auto &f : files[i]) gz[i] |= is_gzip_file(f) ? 1 : 0;
            if (gz[i])
                for (const auto &f : files[i]) {
                    if (!zseq[i].empty()) zseq[i].push_back('N');
                    if (append_fastx(f, zseq[i]) < 0) die("Could not open %s", f.c_str());
                }
        }
        // regions of the staging buffer: file bytes (an upper bound of the sequence bytes) + one separator per
        // file, rounded up to 32
        std::vector<uint64_t> off;
        std::vector<size_t> slot_of, src_of;
        uint64_t tot = 0;
        for (size_t i = 0; i < nb; ++i) {
            if (cached[i]) continue;
            const uint64_t need = gz[i] ? zseq[i].size() + 1 : genome_file_size(o.inpaths[g + i]) + files[i].size() + 1;
            off.push_back(tot);
            tot += (need + 31) & ~(uint64_t)31;
            slot_of.push_back(g + i);
            src_of.push_back(i);
        }
        off.push_back(tot);
        uint8_t *buf = nullptr;
        if (bi == 0) {
            first_stage.reset(new uint8_t[std::max<uint64_t>(tot, 1)]);
            buf = first_stage.get();
        } else {
            if (!pin_taken[x]) {  // adopt the buffer the context thread prepared
                pin[x] = cf.take_stage(x);
                pin_cap[x] = pin[x] ? cf.stage_cap : 0;
                pin_taken[x] = true;
            }
            if (tot > pin_cap[x]) {  // (this buffer's previous batch was retired above)
                if (pin[x]) dsh_free_host(pin[x]);
                pin_cap[x] = tot + (tot >> 4);
                (void)cf.get();
                if (!(pin[x] = (uint8_t *)dsh_alloc_host(pin_cap[x]))) die("could not allocate %zu bytes of pinned host memory", pin_cap[x]);
            }
            buf = pin[x];
        }
        const double t_alloc = now_s();
#pragma omp parallel for schedule(dynamic) num_threads(o.nthreads)
        for (long t = 0; t < (long)slot_of.size(); ++t) {
            const size_t i = src_of[t];
            uint8_t *dst = buf + off[t];
            const size_t cap = (size_t)(off[t + 1] - off[t]);
            size_t len = 0;
            bool raw_ok = !gz[i] && g_device_parse;
            if (raw_ok) {
                // the raw bytes of the genome's files, a '\n' between two files unless the first ends with one (FASTQ counts
                // lines); every file must begin with '>' -- FASTA -- or every file with '@' -- FASTQ in four-line records.
                // What is neither is the host parser's (below), and so is what the device refuses later: a '+' line in a
                // FASTA file, a FASTQ file that does not keep to four lines per record (status != 0: re-parsed when the
                // batch is retired).
                uint8_t kind = 0;
                for (const auto &f : files[i]) {
                    if (len && dst[len - 1] != '\n') {
                        if (len == cap) {  // (a file grew after its region was sized: no room for the separator)
                            raw_ok = false;
                            break;
                        }
                        dst[len++] = '\n';
                    }
                    const size_t at = len;
                    const long rc = read_raw_into(f, dst, cap, len);
                    if (rc == -1) die("Could not open %s", f.c_str());
                    if (len > at && !kind) kind = dst[at];
                    if (rc == -2 || (len > at && (dst[at] != kind || (kind != '>' && kind != '@')))) {
                        raw_ok = false;
                        break;
                    }
                }
                if (raw_ok) {
                    rawkind[i] = 1;
                    rawlen_of[i] = len;
                    continue;  // (no fill: the device pads the DECODED region; raw bytes behind rawlen are never looked at)
                }
                len = 0;
            }
            if (gz[i]) {
                if (!zseq[i].empty()) std::memcpy(dst, zseq[i].data(), zseq[i].size());
                len = zseq[i].size();
                std::vector<uint8_t>().swap(zseq[i]);
            } else {
                for (const auto &f : files[i]) {
                    if (len && len == cap) {  // (the same: no room for the separator)
#pragma omp critical
                        late.push_back(slot_of[t]);
                        break;
                    }
                    if (len) dst[len++] = 'N';
                    const long rc = append_fastx_into(f, dst, cap, len);
                    if (rc == -1) die("Could not open %s", f.c_str());
                    if (rc == -2) {  // the file grew after its region was sized: the whole genome is read growably and sketched
                                     // on its own after the batch (what is staged is a prefix of it: harmless)
#pragma omp critical
                        late.push_back(slot_of[t]);
                        break;
                    }
                }
            }
            std::memset(dst + len, 'N', cap - len);  // invalid bases close every span: no k-mer, harmless
        }
        const double t_parsed = now_s();
        dsh_ctx *ctx = cf.get();
        const double t_ctx = now_s();
        for (size_t i = 0; i < nb; ++i) {
            if (!cached[i] || (skip_cached && !load_cached)) continue;  // `sketch -c`: nothing to do for a cached genome
            int p = 0;
            std::vector<uint8_t> r;
            if (read_hll(fnames[i], r, p) || p != o.S) die("Bad cached sketch %s (expected p=%d)", fnames[i].c_str(), o.S);
            DSH(ctx, dsh_upload_sketches(ctx, r.data(), g + i, 1));
        }
        if (slot_of.size() > status_cap[x]) {
            if (status[x]) dsh_free_host(status[x]);
            status_cap[x] = slot_of.size() + slot_of.size() / 2 + 64;
            if (!(status[x] = (uint32_t *)dsh_alloc_host(status_cap[x] * sizeof(uint32_t)))) die("could not allocate pinned host memory");
        }
        if (!slot_of.empty()) std::memset(status[x], 0, slot_of.size() * sizeof(uint32_t));
        std::vector<uint64_t> rlen(slot_of.size(), 0);
        for (size_t t = 0; t < slot_of.size(); ++t) rlen[t] = rawlen_of[src_of[t]];
        size_t r0 = 0;
        while (r0 < slot_of.size()) {  // consecutive runs of slots of one kind (raw FASTA / parsed sequence) go in one call each
            const int kind = rawkind[src_of[r0]];
            size_t r1 = r0 + 1;
            while (r1 < slot_of.size() && slot_of[r1] == slot_of[r1 - 1] + 1 && rawkind[src_of[r1]] == kind) ++r1;
            if (kind)
                DSH(ctx, dsh_sketch_fastx_batch_async(ctx, buf, off.data() + r0, rlen.data() + r0, (uint32_t)(r1 - r0), slot_of[r0], o.k, o.canon,
                                                      status[x] + r0));
            else
                DSH(ctx, dsh_sketch_batch_async(ctx, buf, off.data() + r0, (uint32_t)(r1 - r0), slot_of[r0], o.k, o.canon));
            r0 = r1;
        }
        for (size_t slot : late) sketch_on_host(ctx, slot);
        Flight &f = fl[x];
        f.slots = slot_of;
        f.fnames.clear();
        f.raw.clear();
        for (size_t t = 0; t < slot_of.size(); ++t) {
            f.fnames.push_back(fnames[src_of[t]]);
            f.raw.push_back((char)rawkind[src_of[t]]);
        }
        DSH(ctx, dsh_event_record(ctx, &f.ticket));
        f.valid = true;
        const double t_enq = now_s();
        if (bi == 0) retire(x);  // (the pageable first buffer is not kept: its copy was synchronous anyway)
        if (g_timing && (bi < 4 || bi % 32 == 0))
            std::fprintf(stderr, "[timing] batch %zu: %zu genomes, %.1f MB staged: retire + pinned alloc %.3f s, stage %.3f s, wait for the context %.3f s, enqueue %.3f s, first-batch retire %.3f s\n",
                         bi, nb, tot / 1e6, t_alloc - t_b0, t_parsed - t_alloc, t_ctx - t_parsed, t_enq - t_ctx, now_s() - t_enq);
        g = e;
        ++bi;
    }
    for (size_t b = bi >= (size_t)kStageBufs ? bi - kStageBufs : 0; b < bi; ++b) retire((int)(b % kStageBufs));  // oldest first
    dsh_ctx *ctx = cf.get();
    DSH(ctx, dsh_wait(ctx));
    for (auto &b : pin)
        if (b) dsh_free_host(b);  // (buffers never adopted are freed by the CtxFuture)
    for (auto &s2 : status)
        if (s2) dsh_free_host(s2);
}

// The end of a subcommand whose outputs are all written and closed.  Tearing the context and the HIP runtime down costs
// 0.1 s (profiles/rd6e/cli_e2e_timing.jsonl: a quarter of `dist` over 1 000 x 5 Mbp), and the kernel driver reclaims
// the device memory, queues and page-locked pages of an exiting process anyway: flush what stdio still holds and leave
// without the destructors.  DSH_FULL_TEARDOWN=1 runs them (leak checkers).
[[maybe_unused]] static void leave(dsh_ctx *ctx)
{
    since_launch("outputs closed");
    std::fflush(nullptr);
    if (std::getenv("DSH_FULL_TEARDOWN")) {
        dsh_destroy(ctx);
        return;
    }
    if (ctx) (void)dsh_synchronize(ctx);
    since_launch("leaving");
    std::fflush(nullptr);
    std::_Exit(EXIT_SUCCESS);
}

static int sketch_main(int argc, char **argv)
{
    Opts o = parse(argc, argv, false);
    if (!o.avoid_sorting) sort_paths_by_fsize(o.inpaths);  // src/dashing.cpp:356-357
    CtxFuture cf(o.device, o.inpaths.size(), o.S, staging_bytes_for(o.inpaths));
    const std::string &output_file = o.out_sizes;  // `sketch -o FILE` (src/dashing.cpp:307-337)
    dsh_ctx *ctx = nullptr;
    if (output_file.empty()) {
        fill_sketches(cf, o, /*write_files=*/true, /*skip_cached=*/o.skip_cached != 0);
        ctx = cf.get();
    } else {
        // all sketches into ONE gz stream + "<FILE>.labels.gz" (src/sketch_and_cmp.h:466-475,529-536);
        // with -c an existing per-genome .hll is read instead of re-sketched (:504-507)
        if (write_labels_gz(output_file + ".labels.gz", o.inpaths)) die("Failed to write sequence labels to file");
        fill_sketches(cf, o, /*write_files=*/false, /*skip_cached=*/o.skip_cached != 0, /*load_cached=*/true);
        ctx = cf.get();
        const size_t n = o.inpaths.size(), m = (size_t)1 << o.S;
        std::vector<uint8_t> all(n * m);
        DSH(ctx, dsh_download_sketches(ctx, 0, n, all.data()));
        if (write_hll_multi(output_file, all.data(), n, o.S, o.estim)) die("Failed to write sketches to file");
    }
    leave(ctx);
    return EXIT_SUCCESS;
}

// ---- utilities on .hll files ----------------------------------------------
// `union` (src/union.cpp:60-107): register-wise maximum of HLL sketch files -> one .hll.
static int union_main(int argc, char **argv)
{
    int level = 6, nthreads = 1;
    std::string opath = "/dev/stdout";
    std::vector<std::string> paths;
    optind = 1;
    for (int c; (c = getopt(argc, argv, "p:o:F:zZ:rHbh?")) >= 0;) {
        switch (c) {
        case 'Z': level = std::atoi(optarg); break;  // (the reference falls through into -o here: a bug we do not keep)
        case 'z': break;                             // output is a gz stream unless -Z 0
        case 'o': opath = optarg; break;
        case 'F': paths = read_paths_file(optarg); break;
        case 'p': nthreads = std::max(1, std::atoi(optarg)); break;
        case 'r': case 'H': case 'b': die("union: only HLL sketches are in scope");
        default:
            std::fprintf(stderr, "Usage: dashing-amd union [-o out.hll] [-F paths.txt] [-p threads] [-Z level] a.hll b.hll ...\n");
            return EXIT_FAILURE;
        }
    }
    for (int i = optind; i < argc; ++i) paths.emplace_back(argv[i]);
    if (paths.empty()) die("require >= 1 paths. See usage.");
    std::vector<std::vector<uint8_t>> acc((size_t)nthreads);
    std::vector<int> ps((size_t)nthreads, -1);
#pragma omp parallel for schedule(dynamic) num_threads(nthreads)
    for (long i = 0; i < (long)paths.size(); ++i) {
        const int t = omp_get_thread_num();
        int p = 0;
        std::vector<uint8_t> r;
        if (read_hll(paths[i], r, p)) die("Could not read sketch %s", paths[i].c_str());
        if (ps[t] < 0) {
            ps[t] = p;
            acc[t].swap(r);
        } else {
            if (p != ps[t]) die("For operator +=: np_ (%d) != other.get_np() (%d)", ps[t], p);
            union_registers(acc[t].data(), r.data(), r.size());
        }
    }
    int p = -1;
    std::vector<uint8_t> *tot = nullptr;
    for (int t = 0; t < nthreads; ++t) {
        if (ps[t] < 0) continue;
        if (!tot) {
            tot = &acc[t];
            p = ps[t];
        } else {
            if (ps[t] != p) die("For operator +=: np_ (%d) != other.get_np() (%d)", p, ps[t]);
            union_registers(tot->data(), acc[t].data(), tot->size());
        }
    }
    if (write_hll(opath, tot->data(), p, ERTL_MLE, ERTL_MLE, false, 0.0, level)) die("Could not open file at %s", opath.c_str());
    return EXIT_SUCCESS;
}

// `view` (src/dashing.cpp:553-557)
static int view_main(int argc, char **argv)
{
    if (argc < 2) die("Usage: dashing-amd view f1.hll [f2.hll ...]. Only HLLs currently supported.");
    for (int i = 1; i < argc; ++i) {
        int p = 0;
        std::vector<uint8_t> r;
        if (read_hll(argv[i], r, p)) die("Could not read sketch %s", argv[i]);
        print_hll(stdout, argv[i], r.data(), p);
    }
    return EXIT_SUCCESS;
}

// `fold` (src/dashing.cpp:558-590): compress a sketch to a smaller precision
static int fold_main(int argc, char **argv)
{
    std::string out = "/dev/stdout", in = "/dev/stdin";
    int destp = -1;
    optind = 1;
    for (int c; (c = getopt(argc, argv, "p:o:h?")) >= 0;) {
        switch (c) {
        case 'o': out = optarg; break;
        case 'p': destp = std::atoi(optarg); break;
        default:
            std::fprintf(stderr, "Usage: dashing-amd fold <flags> [in1.hll]\n-o: Write to <path> instead of stdout\n"
                                 "-p: set destination p [must be smaller than the input sketch\n");
            return EXIT_FAILURE;
        }
    }
    if (argc - optind == 1) in = argv[optind];
    else if (argc - optind > 1) die("Usage: dashing-amd fold <flags> [in1.hll]");
    if (out == "-") out = "/dev/stdout";
    if (in == "-") in = "/dev/stdin";
    int p = 0;
    std::vector<uint8_t> r, f;
    if (read_hll(in, r, p)) die("Could not read sketch %s", in.c_str());
    if (destp <= 0) destp = p - 1;
    if (destp >= p || destp < 4) die("fold: destination p (%d) must be in [4, %d)", destp, p);
    fold_registers(r.data(), p, destp, f);
    if (write_hll(out, f.data(), destp, ERTL_MLE, ERTL_MLE, false, 0.0)) die("Could not write %s", out.c_str());
    return EXIT_SUCCESS;
}

// `printmat` (src/dashing.cpp:425-452): a BINARY distance matrix ('\0', u64 n, packed upper triangle)
// as the full n x n table of DistanceMatrix::printf (distmat/distmat.h:358-381): "%lf" values, tabs
// between, the diagonal is the default value 0.
static int printmat_main(int argc, char **argv)
{
    bool use_scientific = false;
    std::string outpath = "/dev/stdout";
    optind = 1;
    for (int c; (c = getopt(argc, argv, ":o:sh?")) >= 0;) {
        switch (c) {
        case 'o': outpath = optarg; break;
        case 's': use_scientific = true; break;
        default:
            std::fprintf(stderr, "dashing-amd printmat <path to binary file>\n-o\tSpecify output file (default: stdout)\n-s\tEmit in scientific notation\n");
            return EXIT_FAILURE;
        }
    }
    if (optind >= argc) die("dashing-amd printmat <path to binary file>");
    std::FILE *in = std::fopen(std::strcmp(argv[optind], "-") ? argv[optind] : "/dev/stdin", "rb");
    if (!in) die("[print_binary_main] Could not open file at %s", argv[optind]);
    uint64_t n = 0;
    const int magic = std::fgetc(in);
    if (magic != 0 || std::fread(&n, sizeof n, 1, in) != 1) die("%s is not a float distance matrix", argv[optind]);
    const uint64_t total = n ? n * (n - 1) / 2 : 0;
    std::vector<float> tri(std::max<uint64_t>(total, 1));
    if (total && std::fread(tri.data(), sizeof(float), total, in) != total) die("size %llu is not the file size", (unsigned long long)(total * 4 + 9));
    std::fclose(in);
    std::FILE *fp = std::fopen(outpath.c_str(), "wb");
    if (!fp) die("[print_binary_main] Could not open file at %s", outpath.c_str());
    const char *mid = use_scientific ? "%le\t" : "%lf\t", *last = use_scientific ? "%le\n" : "%lf\n";
    for (uint64_t i = 0; i < n; ++i)
        for (uint64_t j = 0; j < n; ++j) {
            double v = 0.;
            if (i != j) {
                const uint64_t a = std::min(i, j), b = std::max(i, j);
                v = (double)tri[dsh_tri_index(n, a, b)];
            }
            std::fprintf(fp, j + 1 == n ? last : mid, v);
        }
    std::fclose(fp);
    return EXIT_SUCCESS;
}

// `hll` (src/hllmain.cpp:4-45): cardinality of the union of the k-mers of all input files --
// every file is sketched into ONE HLL (default p = 24: registers live in HBM, not LDS).
static int hll_main(int argc, char **argv)
{
    int k = 31, S = 24, nthreads = 1, canon = 1, device = 0;
    std::string paths_file;
    if (argc < 2) {
    usage:
        std::fprintf(stderr, "Usage: dashing-amd hll <opts> <paths>\nFlags:\n-k:\tkmer length (Default: 31. Max: 32)\n"
                             "-S:\tsketch size (default: 24). (2^S one-byte registers)\n-p:\tnumber of host threads.\n"
                             "-F:\tPath to file which contains one path per line\n-C:\tdo not canonicalise\n-d:\tGPU ordinal\n");
        return EXIT_FAILURE;
    }
    optind = 1;
    for (int c; (c = getopt(argc, argv, "Cw:s:S:p:k:F:d:tfh?")) >= 0;) {
        switch (c) {
        case 'C': canon = 0; break;
        case 'k': k = std::atoi(optarg); break;
        case 'p': nthreads = std::max(1, std::atoi(optarg)); break;
        case 's': if (optarg && *optarg) die("spaced seeds are out of scope (HLL hot path only)"); break;
        case 'w': if (std::atoi(optarg) > k) die("minimizer windows are out of scope (HLL hot path only)"); break;
        case 'S': S = std::atoi(optarg); break;
        case 'F': paths_file = optarg; break;
        case 'd': device = std::atoi(optarg); break;
        case 't': case 'f': break;
        default: goto usage;
        }
    }
    if (k < 1 || k > 32) die("k must be in [1,32]");
    if (S < 4 || S > 24) die("-S must be in [4,24]");
    std::vector<std::string> inpaths = paths_file.empty() ? std::vector<std::string>(argv + optind, argv + argc) : read_paths_file(paths_file);
    if (inpaths.empty()) goto usage;
    dsh_ctx *ctx = nullptr;
    if (int rc = dsh_create(device, &ctx)) die("[dashing-amd] no usable gfx950 device (dsh_create = %d); there is no CPU fallback", rc);
    DSH(ctx, dsh_sketches_alloc(ctx, 1, S));
    std::fprintf(stderr, "Processing %zu paths with %i threads\n", inpaths.size(), nthreads);
    // batches of files, parsed on the host threads, all max-merged into slot 0
    const size_t batch_bytes = (size_t)512 << 20;
    for (size_t g = 0; g < inpaths.size();) {
        size_t e = g, bytes = 0;
        while (e < inpaths.size() && (e == g || bytes + genome_file_size(inpaths[e]) <= batch_bytes)) bytes += genome_file_size(inpaths[e++]);
        std::vector<std::vector<uint8_t>> seqs(e - g);
#pragma omp parallel for schedule(dynamic) num_threads(nthreads)
        for (long i = 0; i < (long)(e - g); ++i)
            for (const auto &f : split_genome_paths(inpaths[g + i])) {
                if (!seqs[i].empty()) seqs[i].push_back('N');
                if (append_fastx(f, seqs[i]) < 0) die("Could not open %s", f.c_str());
            }
        std::vector<uint8_t> all;
        for (auto &sv : seqs) {
            all.insert(all.end(), sv.begin(), sv.end());
            all.push_back('N');
            std::vector<uint8_t>().swap(sv);
        }
        const uint64_t off[2] = {0, all.size()};
        DSH(ctx, dsh_sketch_batch(ctx, all.data(), off, 1, 0, k, canon, nullptr));
        g = e;
    }
    double est = 0;
    DSH(ctx, dsh_cardinalities(ctx, ERTL_MLE, &est));
    std::fprintf(stdout, "Estimated number of unique exact matches: %lf\n", est);
    dsh_destroy(ctx);
    return EXIT_SUCCESS;
}

// ---- per-record sketches: sketch_by_seq / dist_by_seq (src/dashing.cpp:470-557, src/sketch_and_cmp.h:540-602,
// src/distbyseq.cpp).  Every record of every input, in input order, is one sketch named by its kseq name.
struct Records {
    std::vector<uint8_t> seq;    // the records back to back, no separator
    std::vector<uint64_t> off;   // record r = seq[off[r], off[r+1])
    std::vector<std::string> names;
};

static void read_records(const Opts &o, Records &R)
{
    for (const auto &path : o.inpaths) {
        std::vector<uint64_t> st;
        if (append_fastx_records(path, R.seq, st, R.names) < 0) die("Could not open %s", path.c_str());
        R.off.insert(R.off.end(), st.begin(), st.end());
    }
    R.off.push_back(R.seq.size());
    if (R.names.empty()) die("No sequence records in the inputs.");
}

// "<FILE>.labels.gz" back: one label per line
static std::vector<std::string> read_labels_gz(const std::string &path)
{
    gzFile fp = gzopen(path.c_str(), "rb");
    if (!fp) die("Could not open labels %s", path.c_str());
    std::vector<std::string> v;
    std::string cur;
    char buf[1 << 16];
    while (gzgets(fp, buf, sizeof buf)) {
        cur += buf;
        if (!cur.empty() && cur.back() == '\n') {
            cur.pop_back();
            v.push_back(cur);
            cur.clear();
        }
    }
    if (!cur.empty()) v.push_back(cur);
    gzclose(fp);
    return v;
}

// the records (all, or [rb, re)) into slots [first, first + n): batches of at most kRecordsBatchBytes bases (or one record, if longer)
// through two page-locked buffers that take turns behind tickets, dsh_sketch_records_async (rows overwritten)
static const size_t kRecordsBatchBytes = (size_t)256 << 20;
static void sketch_records_batched(dsh_ctx *ctx, const Records &R, uint64_t first, int k, int canon, size_t rb = 0, size_t re = (size_t)-1)
{
    const size_t n = std::min(re, R.names.size());  // (the records [rb, n) into the slots from `first` on)
    if (rb >= n) return;
    size_t cap = kRecordsBatchBytes;
    for (size_t r = rb; r < n; ++r) cap = std::max<size_t>(cap, R.off[r + 1] - R.off[r]);
    cap = std::min<size_t>(cap, std::max<size_t>(R.seq.size(), 1));
    uint8_t *buf[2] = {(uint8_t *)dsh_alloc_host(cap), (uint8_t *)dsh_alloc_host(cap)};
    if (!buf[0] || !buf[1]) die("could not allocate %zu bytes of pinned host memory", cap);
    uint64_t ticket[2] = {0, 0};
    bool used[2] = {false, false};
    std::vector<uint64_t> off;
    int b = 0;
    for (size_t r0 = rb; r0 < n;) {
        size_t r1 = r0 + 1;
        while (r1 < n && R.off[r1 + 1] - R.off[r0] <= cap && r1 - r0 < ((size_t)1 << 30)) ++r1;
        if (used[b]) DSH(ctx, dsh_event_wait(ctx, ticket[b]));
        const size_t bytes = R.off[r1] - R.off[r0];
        if (bytes) std::memcpy(buf[b], R.seq.data() + R.off[r0], bytes);
        off.assign(R.off.begin() + r0, R.off.begin() + r1 + 1);
        for (auto &x : off) x -= R.off[r0];
        DSH(ctx, dsh_sketch_records_async(ctx, buf[b], off.data(), (uint32_t)(r1 - r0), first + (r0 - rb), k, canon));
        DSH(ctx, dsh_event_record(ctx, &ticket[b]));
        used[b] = true;
        b ^= 1;
        r0 = r1;
    }
    DSH(ctx, dsh_wait(ctx));
    dsh_free_host(buf[0]);
    dsh_free_host(buf[1]);
}


// The same with the parse on the device (dsh_sketch_fastx_records), for plain regular files; compressed
// inputs, pipes and what the device refuses keep the host parser.  Two passes over the inputs, each in batches of raw bytes
// through two page-locked buffers that take turns (the next batch is read while the device works on this one; a file is
// never split: the buffers hold the largest):
//   1. count-only calls: every file's verdict and record count; the refused and the other files are parsed on the host now.
//      Then every file's first slot is known and the matrix is allocated.
//   2. the accepted files again, into their slots, their names read from the staged bytes; the host-parsed files through
//      sketch_records_batched into theirs.
// names and rows ([n][2^S], downloaded) keep the inputs' order and the records' order inside a file.  false: nothing is to
// be used -- a file changed between the passes or was refused only by the full decode (a FASTQ record whose quality has
// another length than its sequence): the caller takes the host path for the whole run.
// Off by default: the host path is, until measurements say otherwise; DSH_DEVICE_PARSE=1 selects
// this one, DSH_HOST_PARSE=1 overrules it as for `sketch` / `dist`.
static const bool g_records_device_parse = g_device_parse && std::getenv("DSH_DEVICE_PARSE") != nullptr;

struct RawBatch {
    size_t f0, f1;  // the inputs [f0, f1), all of them staged
};
static uint64_t raw_region(uint64_t size) { return (size + 1 + 31) & ~(uint64_t)31; }
// runs of consecutive inputs with take[i] set, cut where the regions would exceed cap
static std::vector<RawBatch> raw_batches(const std::vector<uint64_t> &size, const std::vector<char> &take, uint64_t cap)
{
    std::vector<RawBatch> out;
    for (size_t f = 0; f < size.size();) {
        if (!take[f]) {
            ++f;
            continue;
        }
        size_t e = f;
        uint64_t bytes = 0;
        while (e < size.size() && take[e] && (e == f || bytes + raw_region(size[e]) <= cap) && e - f < ((size_t)1 << 20)) bytes += raw_region(size[e++]);
        out.push_back(RawBatch{f, e});
        f = e;
    }
    return out;
}

static bool device_records(const Opts &o, dsh_ctx *ctx, std::vector<std::string> &names, std::vector<uint8_t> &rows)
{
    const double t0 = now_s();
    const size_t nf = o.inpaths.size();
    std::vector<uint64_t> size(nf, 0), count(nf, 0);
    std::vector<char> dev(nf, 0);
    uint64_t cap = kRecordsBatchBytes, total_raw = 0;
    for (size_t f = 0; f < nf; ++f) {
        struct stat st;
        if (::stat(o.inpaths[f].c_str(), &st) != 0) die("Could not open %s", o.inpaths[f].c_str());
        if (!S_ISREG(st.st_mode) || is_gzip_file(o.inpaths[f])) continue;
        dev[f] = 1;
        size[f] = (uint64_t)st.st_size;
        cap = std::max(cap, raw_region(size[f]));
        total_raw += raw_region(size[f]);
    }
    cap = std::min(cap, std::max<uint64_t>(total_raw, 32));
    uint8_t *buf[2] = {(uint8_t *)dsh_alloc_host(cap), (uint8_t *)dsh_alloc_host(cap)};
    if (!buf[0] || !buf[1]) die("could not allocate %llu bytes of pinned host memory", (unsigned long long)cap);
    std::vector<uint64_t> boff[2], blen[2];
    std::atomic<bool> changed{false};  // a file no longer fits the size it had: it grew
    // a batch's raw bytes into buffer x, every file in its region (sized from its stat: nothing is written behind it)
    auto stage = [&](const RawBatch &b, int x) {
        boff[x].assign(1, 0);
        blen[x].clear();
        for (size_t f = b.f0; f < b.f1; ++f) {
            size_t len = 0;
            const long rc = read_raw_into(o.inpaths[f], buf[x] + boff[x].back(), (size_t)size[f], len);
            if (rc == -1) die("Could not open %s", o.inpaths[f].c_str());
            if (rc == -2) changed = true;
            blen[x].push_back(len);
            boff[x].push_back(boff[x].back() + raw_region(size[f]));
        }
    };
    // fn(batch, buffer) for every batch, the next one being read meanwhile; false as soon as fn says so
    auto for_batches = [&](const std::vector<RawBatch> &bs, const std::function<bool(const RawBatch &, int)> &fn) {
        if (bs.empty()) return true;
        stage(bs[0], 0);
        for (size_t i = 0; i < bs.size(); ++i) {
            std::future<void> next;
            if (i + 1 < bs.size()) next = std::async(std::launch::async, [&, i]() { stage(bs[i + 1], (int)((i + 1) & 1)); });
            const bool go = !changed && fn(bs[i], (int)(i & 1));
            if (next.valid()) next.get();
            if (!go || changed) return false;
        }
        return true;
    };
    auto done = [&](bool ok) {
        dsh_free_host(buf[0]);
        dsh_free_host(buf[1]);
        return ok;
    };
    std::vector<uint32_t> status;
    std::vector<uint64_t> nrec;

    // pass 1: verdicts and counts
    if (!for_batches(raw_batches(size, dev, cap), [&](const RawBatch &b, int x) {
            const uint32_t n = (uint32_t)(b.f1 - b.f0);
            status.assign(n, 0);
            nrec.assign(n, 0);
            DSH(ctx, dsh_sketch_fastx_records(ctx, buf[x], boff[x].data(), blen[x].data(), n, nullptr, o.k, o.canon, status.data(), nrec.data(), nullptr));
            for (uint32_t i = 0; i < n; ++i) {
                if (status[i]) dev[b.f0 + i] = 0;
                else count[b.f0 + i] = nrec[i];
            }
            return true;
        }))
        return done(false);
    const double t1 = now_s();
    Records H;  // the records of the files the host parses, file after file
    std::vector<size_t> hfirst(nf + 1, 0);
    for (size_t f = 0; f < nf; ++f) {
        hfirst[f] = H.names.size();
        if (dev[f]) continue;
        std::vector<uint64_t> st;
        if (append_fastx_records(o.inpaths[f], H.seq, st, H.names) < 0) die("Could not open %s", o.inpaths[f].c_str());
        H.off.insert(H.off.end(), st.begin(), st.end());
        count[f] = H.names.size() - hfirst[f];
    }
    hfirst[nf] = H.names.size();
    H.off.push_back(H.seq.size());
    std::vector<uint64_t> slot0(nf + 1, 0);
    for (size_t f = 0; f < nf; ++f) slot0[f + 1] = slot0[f] + count[f];
    const uint64_t total = slot0[nf];
    if (total == 0) die("No sequence records in the inputs.");
    const double t2 = now_s();
    DSH(ctx, dsh_sketches_alloc(ctx, total, o.S));
    names.assign(total, std::string());

    // pass 2: the accepted files into their slots
    std::vector<uint64_t> hdr;
    if (!for_batches(raw_batches(size, dev, cap), [&](const RawBatch &b, int x) {
            const uint32_t n = (uint32_t)(b.f1 - b.f0);
            status.assign(n, 0);
            nrec.assign(n, 0);
            hdr.assign((size_t)(slot0[b.f1] - slot0[b.f0]) + 1, 0);
            const int rc = dsh_sketch_fastx_records(ctx, buf[x], boff[x].data(), blen[x].data(), n, slot0.data() + b.f0, o.k, o.canon, status.data(),
                                                    nrec.data(), hdr.data());
            if (rc == DSH_ERANGE) return false;  // (the file is not what pass 1 counted)
            if (rc) die("[dashing-amd] dsh_sketch_fastx_records failed (%d): %s", rc, dsh_last_error(ctx));
            for (uint32_t i = 0; i < n; ++i) {
                if (status[i]) return false;  // (refused by the full decode only)
                const size_t f = b.f0 + i;
                const char *end = (const char *)buf[x] + boff[x][i] + blen[x][i];
                for (uint64_t r = 0; r < count[f]; ++r) {
                    const char *p = (const char *)buf[x] + hdr[(size_t)(slot0[f] - slot0[b.f0] + r)] + 1;
                    names[(size_t)(slot0[f] + r)].assign(p, fastx_name_len(p, (size_t)(end - p)));
                }
            }
            return true;
        }))
        return done(false);
    const double t3 = now_s();
    size_t ndev = 0;
    for (size_t f = 0; f < nf; ++f) {
        ndev += dev[f] ? 1 : 0;
        if (dev[f]) continue;
        for (size_t r = hfirst[f]; r < hfirst[f + 1]; ++r) names[(size_t)slot0[f] + (r - hfirst[f])] = H.names[r];
        sketch_records_batched(ctx, H, slot0[f], o.k, o.canon, hfirst[f], hfirst[f + 1]);
    }
    rows.resize((size_t)total << o.S);
    DSH(ctx, dsh_download_sketches(ctx, 0, total, rows.data()));
    if (g_timing) {
        std::fprintf(stderr, "[timing] by_seq: %zu files (%llu records) decoded on the device, %zu files (%zu records) on the host\n", ndev,
                     (unsigned long long)(total - H.names.size()), nf - ndev, H.names.size());
        std::fprintf(stderr, "[timing] by_seq: count pass %.3f s, host parse %.3f s, sketch pass %.3f s, host files + download %.3f s\n", t1 - t0,
                     t2 - t1, t3 - t2, now_s() - t3);
    }
    return done(true);
}

// names and rows of every record of the inputs through device_records, on a context of its own; false: take the host path
static bool records_by_device(const Opts &o, std::vector<std::string> &names, std::vector<uint8_t> &rows)
{
    if (!g_records_device_parse) return false;
    const double t0 = now_s();
    dsh_ctx *ctx = nullptr;
    if (int rc = dsh_create(o.device, &ctx)) die("[dashing-amd] no usable gfx950 device (dsh_create = %d); there is no CPU fallback", rc);
    const bool ok = device_records(o, ctx, names, rows);
    dsh_destroy(ctx);
    if (!ok) {
        names.clear();
        rows.clear();
        if (g_timing) std::fprintf(stderr, "[timing] by_seq: an input changed or was refused late; the host parser takes all of them\n");
    } else if (g_timing) {
        std::fprintf(stderr, "[timing] by_seq: records on the device path after %.3f s\n", now_s() - t0);
    }
    return ok;
}

static int sketch_by_seq_main(int argc, char **argv)
{
    Opts o = parse(argc, argv, false);
    const std::string &output_file = o.out_sizes;
    if (output_file.empty()) {
        std::fprintf(stderr, "sketch_by_seq writes every record's sketch into ONE file: -o FILE is required.\n");
        usage("sketch_by_seq");
    }
    Records R;
    std::vector<uint8_t> rows;
    if (records_by_device(o, R.names, rows)) {
        if (write_hll_multi(output_file, rows.data(), R.names.size(), o.S, o.estim)) die("Failed to write sketches to file");
        if (write_labels_gz(output_file + ".labels.gz", R.names)) die("Failed to write sequence labels to file");
        leave(nullptr);
        return EXIT_SUCCESS;
    }
    read_records(o, R);
    const size_t n = R.names.size(), m = (size_t)1 << o.S;
    CtxFuture cf(o.device, n, o.S);
    dsh_ctx *ctx = cf.get();
    sketch_records_batched(ctx, R, 0, o.k, o.canon);
    std::vector<uint8_t> all(n * m);
    DSH(ctx, dsh_download_sketches(ctx, 0, n, all.data()));
    if (write_hll_multi(output_file, all.data(), n, o.S, o.estim)) die("Failed to write sketches to file");
    if (write_labels_gz(output_file + ".labels.gz", R.names)) die("Failed to write sequence labels to file");
    leave(ctx);
    return EXIT_SUCCESS;
}

// ---- dist / dist_by_seq: dist_main (at the end) is the sequence of the phases below -------------------------------
static const char *const kMeasureNames[9] = {"MASH_DIST", "JI", "SIZES", "FULL_MASH_DIST", "FULL_CONTAINMENT_DIST", "CONTAINMENT_INDEX",
                                             "CONTAINMENT_DIST", "SYMMETRIC_CONTAINMENT_INDEX", "SYMMETRIC_CONTAINMENT_DIST"};

// the measures whose smaller value is the closer pair, so that --threshold's test is <=: !measure_descending of ctx.h
static bool is_distance(int result_type)
{
    return result_type == 0 || result_type == 3 || result_type == 4 || result_type == 6 || result_type == 8;
}

// DSH_BLOCK_VALS=N: the row blocks of the streamed triangle hold at most N values, not 256 Mi (no output depends on the cut:
// the tests cross block edges with few inputs this way); anything but a positive integer is ignored
static uint64_t block_vals_from_env()
{
    const char *s = std::getenv("DSH_BLOCK_VALS");
    char *end = nullptr;
    const unsigned long long v = (s && *s >= '0' && *s <= '9') ? std::strtoull(s, &end, 10) : 0;
    return (v && !*end) ? (uint64_t)v : (uint64_t)256 << 20;
}

// what a run of `dist` / `dist_by_seq` carries from phase to phase
struct DistRun {
    Opts o;  // inpaths: the names of the collection in output order -- paths, record names, at last the group names
    bool symmetric = true;
    uint64_t block_vals = 0;    // cap of a row block (for_row_blocks)
    Records R;                  // dist_by_seq: the records ...
    std::vector<uint8_t> pre;   // ... or, with --presketched, the sketch_by_seq stream
    std::vector<uint32_t> hist_labels, extend_labels;  // --histogram-labels, --extend
    std::vector<std::pair<std::string, std::string>> pair_names;  // --pairs: the listed names, their slots, the measures
    std::vector<uint32_t> lhs, rhs;
    std::vector<int> pair_types;
    std::vector<std::string> group_names;  // --groups: in order of first appearance, and the members of each as input slots
    std::vector<uint64_t> group_ptr;
    std::vector<uint32_t> group_members;
    size_t n = 0, nq = 0;  // sketches in all; the last nq are the queries
    dsh_ctx *ctx = nullptr;
};

// --measures LIST, or the one measure the other flags select
static std::vector<int> parse_measures(const Opts &o)
{
    std::vector<int> types;
    if (o.measures.empty()) types.push_back(o.result_type);
    for (size_t b = 0; b <= o.measures.size() && !o.measures.empty();) {  // (an empty element, a trailing comma included, is no measure)
        const size_t e = std::min(o.measures.find(',', b), o.measures.size());
        const std::string name = o.measures.substr(b, e - b);
        int t = 0;
        while (t < 9 && name != kMeasureNames[t]) ++t;
        if (t == 9) die("--measures: unknown measure '%s'", name.c_str());
        types.push_back(t);
        b = e + 1;
    }
    if (types.empty() || types.size() > 9) die("--measures takes one to nine names.");
    return types;
}

// Phase 1, behind parse: every refusal the options alone decide, before a record, label, pair or group file is opened.  In this
// order: a command line with several conflicts names the first of them.  (What needs a file's content is refused where the
// file is read: label counts against n, p against -S, names that are no inputs.)
static void refuse_conflicts(const Opts &o, bool by_seq)
{
    const bool with_pairs = !o.pairs_file.empty();
    if (by_seq && !o.groups_file.empty()) die("--groups does not go with dist_by_seq: the groups name input files.");
    if (by_seq) {
        if (!o.querypaths.empty()) die("dist_by_seq does not take -Q: every record is compared with every other.");
        if (o.devices.size() > 1) die("dist_by_seq runs on one device: --ngpus / --devices are not supported.");
        if (o.cache) die("dist_by_seq does not take -W: records have no per-genome sketch files to cache.");
        if (o.presketched && o.inpaths.size() != 1) die("dist_by_seq --presketched takes ONE sketch_by_seq file.");
    }
    if (o.has_threshold) {
        if (o.nneighbors) die("--threshold does not go with --nearest-neighbors: choose one selection.");
        if (o.fmt == UPPER_TRIANGULAR) die("--threshold does not go with -U: a PHYLIP matrix is dense.");
        if (o.fmt == FULL_TSV) die("--threshold does not go with -T: a full TSV matrix is dense.");
        if (o.devices.size() > 1) die("--threshold runs on one device: --ngpus / --devices are not supported.");
    }
    if (o.has_cluster) {
        if (o.has_threshold) die("--cluster does not go with --threshold: choose the clusters or the pairs.");
        if (o.nneighbors) die("--cluster does not go with --nearest-neighbors: choose one selection.");
        if (with_pairs) die("--cluster does not go with --pairs: the clusters are those of all pairs.");
        if (!o.querypaths.empty()) die("--cluster does not go with -Q: every input is clustered with every other.");
        if (o.fmt == UPPER_TRIANGULAR) die("--cluster does not go with -U: the output is one line per input.");
        if (o.fmt == FULL_TSV) die("--cluster does not go with -T: the output is one line per input.");
        if (o.devices.size() > 1 || o.rccl) die("--cluster runs on one device: --ngpus / --devices are not supported.");
    }
    if (o.linkage >= 0 && !o.has_cluster) die("--linkage goes with --cluster only.");
    if (o.linkage == DSH_LINKAGE_AVERAGE && o.result_type == DSH_SIZES) die("--linkage average does not go with --sizes: it judges values in (-2, 2).");
    if (o.has_min_pts && !o.has_cluster) die("--min-pts goes with --cluster only.");
    if (o.has_min_pts && o.linkage > DSH_LINKAGE_SINGLE) die("--min-pts does not go with --linkage complete or average: density clusters are components of cores.");
    if (o.has_reps) {  // (what --cluster refuses, and --cluster)
        if (o.has_cluster) die("--representatives does not go with --cluster: choose the representatives or the components.");
        if (o.has_threshold) die("--representatives does not go with --threshold: choose the representatives or the pairs.");
        if (o.nneighbors) die("--representatives does not go with --nearest-neighbors: choose one selection.");
        if (with_pairs) die("--representatives does not go with --pairs: the representatives are those of all pairs.");
        if (!o.querypaths.empty()) die("--representatives does not go with -Q: every input is tested against every earlier one.");
        if (o.fmt == UPPER_TRIANGULAR) die("--representatives does not go with -U: the output is one line per input.");
        if (o.fmt == FULL_TSV) die("--representatives does not go with -T: the output is one line per input.");
        if (o.devices.size() > 1 || o.rccl) die("--representatives runs on one device: --ngpus / --devices are not supported.");
    }
    if (o.has_hist) {
        if (o.has_threshold) die("--histogram does not go with --threshold: choose the distribution or the pairs.");
        if (o.has_cluster) die("--histogram does not go with --cluster: choose the distribution or the clusters.");
        if (o.has_reps) die("--histogram does not go with --representatives: choose the distribution or the representatives.");
        if (o.nneighbors) die("--histogram does not go with --nearest-neighbors: choose one selection.");
        if (with_pairs) die("--histogram does not go with --pairs: the distribution is that of all pairs.");
        if (o.fmt == UPPER_TRIANGULAR) die("--histogram does not go with -U: the output is one line per class.");
        if (o.fmt == FULL_TSV) die("--histogram does not go with -T: the output is one line per class.");
        if (o.devices.size() > 1 || o.rccl) die("--histogram runs on one device: --ngpus / --devices are not supported.");
    }
    if (o.has_curve) {
        if (by_seq) die("--union-curve does not go with dist_by_seq: the curve is that of input files.");
        if (o.has_threshold) die("--union-curve does not go with --threshold: the curve compares no pairs.");
        if (o.has_cluster) die("--union-curve does not go with --cluster: choose the curve or the clusters.");
        if (o.has_reps) die("--union-curve does not go with --representatives: choose the curve or the representatives.");
        if (o.nneighbors) die("--union-curve does not go with --nearest-neighbors: choose one selection.");
        if (o.has_hist) die("--union-curve does not go with --histogram: choose the curve or the distribution.");
        if (o.has_mst) die("--union-curve does not go with --mst: choose the curve or the tree.");
        if (with_pairs) die("--union-curve does not go with --pairs: the curve compares no pairs.");
        if (!o.groups_file.empty()) die("--union-curve does not go with --groups: the curve is that of the inputs.");
        if (!o.querypaths.empty()) die("--union-curve does not go with -Q: the curve takes every input in turn.");
        if (o.fmt == UPPER_TRIANGULAR) die("--union-curve does not go with -U: the output is one line per input.");
        if (o.fmt == FULL_TSV) die("--union-curve does not go with -T: the output is one line per input.");
        if (o.devices.size() > 1 || o.rccl) die("--union-curve runs on one device: --ngpus / --devices are not supported.");
    }
    if (o.has_curve_perms && !o.has_curve) die("--curve-permutations goes with --union-curve only.");
    if (o.has_curve_seed && !o.has_curve) die("--curve-seed goes with --union-curve only.");
    if (o.has_mst) {  // (what --cluster refuses, and the other selections)
        if (o.has_cluster) die("--mst does not go with --cluster: the tree gives the clusters at every threshold.");
        if (o.has_reps) die("--mst does not go with --representatives: choose the tree or the representatives.");
        if (o.has_hist) die("--mst does not go with --histogram: choose the tree or the distribution.");
        if (o.has_stats) die("--mst does not go with --stats: the tree is no labelling.");
        if (o.has_threshold) die("--mst does not go with --threshold: choose the tree or the pairs (--mst-cutoff bounds the tree's edges).");
        if (o.nneighbors) die("--mst does not go with --nearest-neighbors: choose one selection.");
        if (with_pairs) die("--mst does not go with --pairs: the tree is that of all pairs.");
        if (!o.querypaths.empty()) die("--mst does not go with -Q: every input is joined with every other.");
        if (o.fmt == UPPER_TRIANGULAR) die("--mst does not go with -U: the output is one line per edge.");
        if (o.fmt == FULL_TSV) die("--mst does not go with -T: the output is one line per edge.");
        if (o.devices.size() > 1 || o.rccl) die("--mst runs on one device: --ngpus / --devices are not supported.");
    }
    if (o.has_mst_cutoff && !o.has_mst) die("--mst-cutoff goes with --mst only.");
    if (o.dendrogram && !o.has_mst) die("--dendrogram goes with --mst only.");
    if (!o.hist_labels_file.empty() && !o.has_hist) die("--histogram-labels goes with --histogram only.");
    if (o.has_assign && !o.has_reps && !o.has_min_pts) die("--assign goes with --representatives only.");
    if (o.has_stats && !o.has_cluster && !o.has_reps) die("--stats goes with --cluster or --representatives only.");
    if (o.has_stats && o.result_type == DSH_SIZES) die("--stats does not go with --sizes: set sizes have no mean or worst value inside a group.");
    if (!o.extend_file.empty()) {
        if (!o.has_reps) die("--extend goes with --representatives only.");
        if (!o.avoid_sorting) die("--extend needs --avoid-sorting: sorting by size would interleave the old inputs and the new.");
    }
    if (!o.measures.empty() && !with_pairs) die("--measures goes with --pairs only.");
    if (with_pairs) {
        if (!o.querypaths.empty()) die("--pairs does not go with -Q: the list names the pairs, from all inputs.");
        if (o.nneighbors) die("--pairs does not go with --nearest-neighbors: choose one selection.");
        if (o.has_threshold) die("--pairs does not go with --threshold: choose one selection.");
        if (o.fmt == BINARY) die("--pairs does not go with -b: the output is one text line per pair.");
        if (o.devices.size() > 1) die("--pairs runs on one device: --ngpus / --devices are not supported.");
    }
    if (!o.groups_file.empty()) {
        if (with_pairs) die("--groups does not go with --pairs: a pair list names inputs, not groups.");
        if (!o.querypaths.empty()) die("--groups does not go with -Q: every group is compared with every other.");
        if (o.devices.size() > 1 || o.rccl) die("--groups runs on one device: --ngpus / --devices are not supported.");
    }
}

// Phase 2 of dist_by_seq: the records, or a sketch_by_seq file, take the place of the genomes and their names that of the paths
static void read_records_or_presketched(DistRun &r)
{
    Opts &o = r.o;
    if (o.presketched) {
        int p = 0;
        size_t cnt = 0;
        if (read_hll_multi(o.inpaths[0], r.pre, p, cnt)) die("Could not read sketches from %s", o.inpaths[0].c_str());
        if (p != o.S) die("Sketches in %s have p=%d but -S is %d", o.inpaths[0].c_str(), p, o.S);
        r.R.names = read_labels_gz(o.inpaths[0] + ".labels.gz");
        if (r.R.names.size() != cnt) die("%s holds %zu sketches but its labels %zu names", o.inpaths[0].c_str(), cnt, r.R.names.size());
    } else if (!records_by_device(o, r.R.names, r.pre)) {  // (device-parsed records arrive as rows, like a sketch_by_seq file's)
        read_records(o, r.R);
    }
    o.inpaths = r.R.names;
}

// Phase 3: the files that options name, but for --groups' (parse_groups_file: its lines are checked against the inputs)
static void read_option_files(DistRun &r)
{
    const Opts &o = r.o;
    if (!o.hist_labels_file.empty()) r.hist_labels = read_labels_binary("--histogram-labels", o.hist_labels_file);
    // --extend: u64 n_old, u64 n_reps, u32 labels[n_old], as --representatives -b wrote it for the first n_old inputs
    if (!o.extend_file.empty()) {
        r.extend_labels = read_labels_binary("--extend", o.extend_file);
        if (o.groups_file.empty() && r.extend_labels.size() > o.inpaths.size())
            die("--extend: %s labels %zu inputs but this run has only %zu", o.extend_file.c_str(), r.extend_labels.size(), o.inpaths.size());
    }
    if (!o.pairs_file.empty()) {
        const long bad = read_pairs_file(o.pairs_file, r.pair_names);
        if (bad < 0) die("Could not open %s", o.pairs_file.c_str());
        if (bad > 0) die("%s, line %ld: a pair is two names separated by one tab.", o.pairs_file.c_str(), bad);
    }
}

// Phase 4: output order, the queries behind the references (src/distmain.cpp:120-133)
static void order_paths(DistRun &r)
{
    Opts &o = r.o;
    // asymmetric measure without -Q: all references are also the queries
    // (--cluster, --representatives and --histogram take every pair once, in the triangle's orientation: no query/reference format
    // of their own making for them)
    r.symmetric = o.has_cluster || o.has_reps || o.has_hist || o.has_mst || o.has_curve || !(o.result_type == 4 || o.result_type == 5 || o.result_type == 6);  // src/dashing.h:389-399
    if (o.querypaths.empty() && !r.symmetric && o.pairs_file.empty() && o.groups_file.empty()) {  // (a pair list names its own pairs, each in one orientation; the groups take their turn in union_groups)
        o.querypaths = o.inpaths;
        std::fprintf(stderr, "Note: No query files provided, but an asymmetric distance was requested. Switching to a query/reference format with all references as queries.\n");
    }
    if (!o.presketched && !o.avoid_sorting) {
        sort_paths_by_fsize(o.inpaths);
        sort_paths_by_fsize(o.querypaths);
    }
    r.nq = o.querypaths.size();
    for (auto &q : o.querypaths) o.inpaths.push_back(q);
    r.n = o.inpaths.size();
}

// Phase 5: names to slots, before anything is sketched (a name given twice: its first slot)
static std::unordered_map<std::string, uint32_t> slots_by_name(const std::vector<std::string> &names)
{
    std::unordered_map<std::string, uint32_t> slot_of;
    for (size_t i = names.size(); i-- > 0;) slot_of[names[i]] = (uint32_t)i;
    return slot_of;
}

// --groups FILE: name<TAB>group per line, every input exactly once
static void parse_groups_file(DistRun &r)
{
    const Opts &o = r.o;
    const size_t n = r.n;
    const auto slot_of = slots_by_name(o.inpaths);
    std::unordered_map<std::string, uint32_t> group_of;
    if (slot_of.size() != n) die("--groups: an input is given twice.");
    std::vector<uint32_t> gid(n, ~0u);
    std::ifstream gf(o.groups_file);
    if (!gf) die("Could not open %s", o.groups_file.c_str());
    std::string line;
    for (long ln = 1; std::getline(gf, line); ++ln) {
        if (!line.empty() && line.back() == '\r') line.pop_back();
        if (line.empty()) continue;
        const size_t tab = line.find('\t');
        if (tab == std::string::npos || tab == 0 || tab + 1 == line.size() || line.find('\t', tab + 1) != std::string::npos)
            die("%s, line %ld: a line is a name and a group separated by one tab.", o.groups_file.c_str(), ln);
        const std::string name = line.substr(0, tab), grp = line.substr(tab + 1);
        const auto it = slot_of.find(name);
        if (it == slot_of.end()) die("%s: '%s' is not one of the inputs.", o.groups_file.c_str(), name.c_str());
        if (gid[it->second] != ~0u) die("%s: '%s' is named twice.", o.groups_file.c_str(), name.c_str());
        const auto g = group_of.emplace(grp, (uint32_t)r.group_names.size());
        if (g.second) r.group_names.push_back(grp);
        gid[it->second] = g.first->second;
    }
    for (size_t i = 0; i < n; ++i)
        if (gid[i] == ~0u) die("%s: the input '%s' has no group.", o.groups_file.c_str(), o.inpaths[i].c_str());
    const size_t ng = r.group_names.size();
    r.group_ptr.assign(ng + 1, 0);
    for (size_t i = 0; i < n; ++i) ++r.group_ptr[gid[i] + 1];
    for (size_t g = 0; g < ng; ++g) r.group_ptr[g + 1] += r.group_ptr[g];
    r.group_members.resize(n);
    std::vector<uint64_t> fill(r.group_ptr.begin(), r.group_ptr.end() - 1);
    for (size_t i = 0; i < n; ++i) r.group_members[fill[gid[i]]++] = (uint32_t)i;
}

// --pairs: the slots of the listed names
static void look_up_pairs(DistRun &r)
{
    const Opts &o = r.o;
    const auto slot_of = slots_by_name(o.inpaths);
    r.lhs.resize(r.pair_names.size());
    r.rhs.resize(r.pair_names.size());
    for (size_t x = 0; x < r.pair_names.size(); ++x) {
        const auto a = slot_of.find(r.pair_names[x].first), b = slot_of.find(r.pair_names[x].second);
        if (a == slot_of.end()) die("%s: '%s' is not one of the inputs.", o.pairs_file.c_str(), r.pair_names[x].first.c_str());
        if (b == slot_of.end()) die("%s: '%s' is not one of the inputs.", o.pairs_file.c_str(), r.pair_names[x].second.c_str());
        r.lhs[x] = a->second, r.rhs[x] = b->second;
    }
}

// Phase 6, loader 1 of 3 (the third is fill_sketches): the records into [0, nr) and, as queries of an asymmetric measure,
// once more into [nr, n)
static void load_records(dsh_ctx *ctx, const DistRun &r)
{
    const Opts &o = r.o;
    const size_t nrec = r.R.names.size();
    for (size_t s0 = 0; s0 < r.n; s0 += nrec) {
        if (!r.pre.empty()) DSH(ctx, dsh_upload_sketches(ctx, r.pre.data(), s0, nrec));
        else sketch_records_batched(ctx, r.R, s0, o.k, o.canon);
    }
}

// Loader 2: .hll files (sketch.read(path), src/sketch_and_cmp.h:318-324), read on all host threads into a staging matrix,
// uploaded in batches
static void load_hll_files(dsh_ctx *ctx, const Opts &o, size_t n)
{
    const size_t m = (size_t)1 << o.S, batch = std::max<size_t>(1, ((size_t)256 << 20) / m);
    std::vector<uint8_t> stage(std::min(n, batch) * m);
    // a file sketched at a higher precision than -S is folded on the device (dsh_upload_sketches_folded): its
    // registers wait here until the batch is read, then go run by run of equal p.  At most 256 MiB of them are held: a
    // batch ends before the file that would exceed that
    std::vector<std::vector<uint8_t>> hi(std::min(n, batch));
    std::vector<int> hi_p(std::min(n, batch));
    std::vector<uint8_t> run;
    for (size_t b0 = 0, b1; b0 < n; b0 = b1) {
        b1 = std::min(n, b0 + batch);
        std::atomic<size_t> held{0};
        std::atomic<int64_t> cut{(int64_t)b1};
#pragma omp parallel for schedule(dynamic, 16) num_threads(o.nthreads)
        for (int64_t i = (int64_t)b0; i < (int64_t)b1; ++i) {
            if (i >= cut.load()) continue;  // behind a file that did not fit: the next batch
            int p = 0;
            std::vector<uint8_t> r;
            if (read_hll(o.inpaths[i], r, p)) die("Could not read sketch %s", o.inpaths[i].c_str());
            if (p < o.S) die("Sketch %s has p=%d but -S is %d", o.inpaths[i].c_str(), p, o.S);
            hi_p[i - b0] = p;
            if (p == o.S) {
                std::memcpy(stage.data() + (size_t)(i - (int64_t)b0) * m, r.data(), m);
            } else if (held.fetch_add(r.size()) + r.size() > ((size_t)256 << 20) && i > (int64_t)b0) {
                for (int64_t c = cut.load(); i < c && !cut.compare_exchange_weak(c, i);) {}
            } else {
                hi[i - b0].swap(r);
            }
        }
        b1 = (size_t)cut.load();
        for (size_t i = b0; i < b1;) {
            const int p = hi_p[i - b0];
            const size_t mp = (size_t)1 << p, cap = std::max<size_t>(1, ((size_t)256 << 20) / mp);
            size_t j = i + 1;
            while (j < b1 && hi_p[j - b0] == p && j - i < cap) ++j;
            if (p == o.S) {
                DSH(ctx, dsh_upload_sketches(ctx, stage.data() + (i - b0) * m, i, j - i));
            } else {
                run.resize((j - i) * mp);
                for (size_t x = i; x < j; ++x) std::memcpy(run.data() + (x - i) * mp, hi[x - b0].data(), mp);
                DSH(ctx, dsh_upload_sketches_folded(ctx, run.data(), p, i, j - i));
            }
            i = j;
        }
        for (auto &h : hi) std::vector<uint8_t>().swap(h);
    }
}

// Phase 7, --groups: the unions go into a device buffer that a second context takes as its sketch matrix; from here on the
// groups are the collection.  An asymmetric measure wants every reference once more as a query: the groups twice
static void union_groups(DistRun &r)
{
    Opts &o = r.o;
    const size_t ng = r.group_names.size(), copies = r.symmetric ? 1 : 2;
    if (!r.symmetric) {
        std::fprintf(stderr, "Note: No query files provided, but an asymmetric distance was requested. Switching to a query/reference format with all references as queries.\n");
        const std::vector<uint32_t> once(r.group_members);
        for (size_t g = 0; g < ng; ++g) {
            r.group_names.push_back(r.group_names[g]);
            r.group_ptr.push_back(r.group_ptr.back() + (r.group_ptr[g + 1] - r.group_ptr[g]));
            r.group_members.insert(r.group_members.end(), once.begin() + (long)r.group_ptr[g], once.begin() + (long)r.group_ptr[g + 1]);
        }
        r.nq = ng;
    }
    void *d_union = nullptr;
    if (hipSetDevice(o.device) != hipSuccess || hipMalloc(&d_union, std::max<size_t>((copies * ng) << o.S, 256)) != hipSuccess)
        die("[dashing-amd] no device memory for the unions of %zu groups", ng);
    DSH(r.ctx, dsh_union_groups_device(r.ctx, r.group_ptr.data(), r.group_members.data(), copies * ng, d_union));
    dsh_ctx *gctx = nullptr;
    if (int rc = dsh_create(o.device, &gctx)) die("[dashing-amd] dsh_create(device %d) = %d", o.device, rc);
    DSH(gctx, dsh_attach_device_sketches(gctx, d_union, copies * ng, o.S));
    dsh_destroy(r.ctx);
    r.ctx = gctx;  // (the buffer lives as long as the process)
    o.inpaths = r.group_names;
    r.n = copies * ng;
}

// Phase 8: sizes (src/sketch_and_cmp.h:372-385)
static void write_sizes(const DistRun &r, std::FILE *ofp)
{
    std::vector<double> card(std::max<size_t>(r.n, 1));
    DSH(r.ctx, dsh_cardinalities(r.ctx, r.o.estim, card.data()));
    emit_sizes(ofp, r.o.inpaths, card.data());
    if (ofp != stdout) std::fclose(ofp);
}

// ---- Phase 9: one emitter per selection, each given the run (context, options, names = o.inpaths, n, nq) and the output file
static void check_query_count(size_t n, size_t nq)
{
    if (nq >= n && nq) die("Wrong number of query/references. (ip size: %zu, nq: %zu", n, nq);
}

static uint64_t tri_total(size_t n)
{
    return n ? (uint64_t)n * (n - 1) / 2 : 0;
}

// The rows [r0, r1) of the n-sketch triangle in blocks of at most block_vals values (a block is at least one row), each handed
// to sink(first row, end row, values, span) in order.  Two page-locked ping-pong buffers, asynchronous C-ABI calls: block b+1 is
// enqueued (compute + copy into its buffer, which the sink left in the previous iteration) and its ticket recorded before block b
// is awaited, so the GPU works while the sink formats / writes -- dist_loop's dps[i & 1] scheme (src/sketch_and_cmp.h:804-816)
// without the writer thread.  Blocks are large by default (256 Mi values) so that each one is a row range the library lays its
// plane matrix out for (few planes per tile, values at their final positions).
template <class Sink>
static void for_row_blocks(dsh_ctx *ctx, const Opts &o, uint64_t n, uint64_t r0, uint64_t r1, uint64_t block_vals, Sink sink)
{
    std::vector<uint64_t> cuts{r0};
    while (cuts.back() < r1) {
        const uint64_t rb = cuts.back();
        uint64_t re = rb + 1;
        while (re < r1 && dsh_tri_span(n, rb, re + 1) <= block_vals) ++re;
        cuts.push_back(re);
    }
    uint64_t cap = 1;
    for (size_t b = 0; b + 1 < cuts.size(); ++b) cap = std::max<uint64_t>(cap, dsh_tri_span(n, cuts[b], cuts[b + 1]));
    float *bufs[2] = {nullptr, nullptr};
    for (int w = 0; w < (cuts.size() > 2 ? 2 : 1); ++w)
        if (!(bufs[w] = (float *)dsh_alloc_host(cap * sizeof(float)))) die("could not allocate %llu bytes of pinned host memory", (unsigned long long)(cap * sizeof(float)));
    const size_t nblocks = cuts.size() - 1;
    if (g_timing)
        std::fprintf(stderr, "[timing] rows [%llu, %llu): %zu blocks of at most %llu values, %d buffers\n", (unsigned long long)r0, (unsigned long long)r1, nblocks,
                     (unsigned long long)block_vals, bufs[1] ? 2 : 1);
    std::vector<uint64_t> ticket(nblocks + 1, 0);
    auto enqueue = [&](size_t b) {
        DSH(ctx, dsh_dist_rows_async(ctx, o.estim, o.result_type, o.k, cuts[b], cuts[b + 1], bufs[b & 1]));
        DSH(ctx, dsh_event_record(ctx, &ticket[b]));
    };
    if (nblocks) enqueue(0);
    for (size_t b = 0; b < nblocks; ++b) {
        if (b + 1 < nblocks) enqueue(b + 1);  // its kernels fill the library's other device buffer while block b is still copied out
        DSH(ctx, dsh_event_wait(ctx, ticket[b]));  // block b has arrived in bufs[b & 1]
        sink(cuts[b], cuts[b + 1], (const float *)bufs[b & 1], dsh_tri_span(n, cuts[b], cuts[b + 1]));
    }
    for (auto &b : bufs) dsh_free_host(b);
}

// a context on device `device` that holds the n sketches `all` was downloaded as: what a further device of a multi-device run
// computes its rows from
static dsh_ctx *secondary_context(int device, const std::vector<uint8_t> &all, size_t n, int S)
{
    dsh_ctx *c = nullptr;
    if (int rc = dsh_create(device, &c)) die("[dashing-amd] dsh_create(device %d) = %d", device, rc);
    DSH(c, dsh_sketches_alloc(c, n, S));
    DSH(c, dsh_upload_sketches(c, all.data(), 0, n));
    return c;
}

// --pairs: only the listed pairs (dsh_dist_pairs): the first name is lhs, the second rhs of result_cmp
static void emit_pairs(const DistRun &r, std::FILE *fp)
{
    const Opts &o = r.o;
    const size_t np = r.pair_names.size(), nt = r.pair_types.size();
    std::vector<float> vals(std::max<size_t>(np * nt, 1));
    DSH(r.ctx, dsh_dist_pairs(r.ctx, o.estim, r.pair_types.data(), (uint32_t)nt, o.k, r.lhs.data(), r.rhs.data(), np, vals.data()));
    std::string s;
    char num[64];
    for (size_t x = 0; x < np; ++x) {
        s = r.pair_names[x].first;
        s += '\t';
        s += r.pair_names[x].second;
        for (size_t t = 0; t < nt; ++t) s.append(num, (size_t)std::snprintf(num, sizeof num, "\t%.6g", (double)vals[t * np + x]));  // --threshold's number format
        s += '\n';
        std::fwrite(s.data(), 1, s.size(), fp);
    }
}

// --cluster: the connected components of the pairs that pass (dsh_cluster_threshold); --representatives: the greedy pass in
// output order (dsh_greedy_threshold / dsh_greedy_extend).  No pair leaves the device.  One layout for both: the header word and
// the count differ, and --representatives' text has the value column
static void emit_labelling(const DistRun &r, std::FILE *fp)
{
    const Opts &o = r.o;
    const size_t n = r.n;
    const std::vector<std::string> &names = o.inpaths;
    const bool reps = o.has_reps;
    const float t = reps ? o.reps_t : o.cluster_t;
    std::vector<uint32_t> labels(std::max<size_t>(n, 1));
    uint64_t count = 0;
    const bool linked = !reps && o.linkage > DSH_LINKAGE_SINGLE;  // (single, given or not: the components, every byte as before)
    if (linked) {
        DSH(r.ctx, dsh_linkage_threshold(r.ctx, o.estim, o.result_type, o.k, t, o.linkage, labels.data(), &count));
    } else if (!reps) {
        DSH(r.ctx, dsh_cluster_threshold(r.ctx, o.estim, o.result_type, o.k, t, labels.data(), &count));
    } else {
        if (r.extend_labels.size() > n) die("--extend: %s labels %zu inputs but this run has only %zu", o.extend_file.c_str(), r.extend_labels.size(), n);
        if (o.has_assign || !o.extend_file.empty())
            DSH(r.ctx, dsh_greedy_extend(r.ctx, o.estim, o.result_type, o.k, t, o.assign_mode, r.extend_labels.size(),
                                         r.extend_labels.empty() ? nullptr : r.extend_labels.data(), labels.data(), &count));
        else
            DSH(r.ctx, dsh_greedy_threshold(r.ctx, o.estim, o.result_type, o.k, t, labels.data(), &count));
    }
    GroupStats gs;
    if (o.has_stats) gs.compute(r.ctx, o, labels, n);
    if (o.fmt == BINARY) {
        const uint64_t hdr[2] = {(uint64_t)n, count};
        if (std::fwrite(hdr, sizeof(uint64_t), 2, fp) != 2 || std::fwrite(labels.data(), sizeof(uint32_t), n, fp) != n) die("Error writing to binary file");
        if (o.has_stats) gs.write_binary(fp, n);
        return;
    }
    std::fprintf(fp, "#%s\t%s\t%s\t%.6g%s\n", reps ? "Representatives" : "Cluster", kMeasureNames[o.result_type], is_distance(o.result_type) ? "<=" : ">=",
                 (double)t, !linked ? "" : o.linkage == DSH_LINKAGE_COMPLETE ? "\tcomplete" : "\taverage");  // --threshold's number format
    // --representatives: the value of every non-representative against its label: ONE list of pairs (lhs = the input, rhs =
    // its representative), by dsh_dist_pairs' contract bit for bit the triangle's value
    std::vector<uint32_t> plhs, prhs;
    for (size_t x = 0; reps && x < n; ++x)
        if (labels[x] != x) plhs.push_back((uint32_t)x), prhs.push_back(labels[x]);
    std::vector<float> pv(std::max<size_t>(plhs.size(), 1));
    const int type = o.result_type;
    if (!plhs.empty()) DSH(r.ctx, dsh_dist_pairs(r.ctx, o.estim, &type, 1, o.k, plhs.data(), prhs.data(), plhs.size(), pv.data()));
    // clusters are numbered by ascending representative: a label is its cluster's first member (a representative comes
    // before its members), so the numbers are handed out in one pass
    std::vector<uint32_t> index(std::max<size_t>(n, 1));
    uint32_t next = 0;
    size_t at = 0;
    std::string s;
    char num[64];
    for (size_t x = 0; x < n; ++x) {
        if (labels[x] == x) index[x] = next++;
        s = names[x];
        s.append(num, (size_t)std::snprintf(num, sizeof num, "\t%u\t", index[labels[x]]));
        s += names[labels[x]];
        if (reps && labels[x] == x) s += "\t-";
        else if (reps) s.append(num, (size_t)std::snprintf(num, sizeof num, "\t%.6g", (double)pv[at++]));
        if (o.has_stats) gs.append_fields(s, x, names);
        s += '\n';
        std::fwrite(s.data(), 1, s.size(), fp);
    }
}

// --cluster FLOAT --min-pts N: the density clusters of the pairs that pass (dsh_dbscan_threshold).  No pair leaves the device.
// A label is its cluster's smallest CORE, which may come behind a border it labels: the clusters are numbered in a pass of
// their own, by ascending label
static void emit_dbscan(const DistRun &r, std::FILE *fp)
{
    const Opts &o = r.o;
    const size_t n = r.n;
    const std::vector<std::string> &names = o.inpaths;
    std::vector<uint32_t> labels(std::max<size_t>(n, 1)), degree(std::max<size_t>(n, 1));
    std::vector<uint8_t> kind(std::max<size_t>(n, 1));
    uint64_t count = 0, noise = 0;
    DSH(r.ctx, dsh_dbscan_threshold(r.ctx, o.estim, o.result_type, o.k, o.cluster_t, o.min_pts, o.assign_mode, labels.data(), kind.data(),
                                    degree.data(), &count, &noise));
    GroupStats gs;
    if (o.has_stats) gs.compute(r.ctx, o, labels, n);
    if (o.fmt == BINARY) {
        const uint64_t hdr[2] = {(uint64_t)n, count};
        if (std::fwrite(hdr, sizeof(uint64_t), 2, fp) != 2 || std::fwrite(labels.data(), sizeof(uint32_t), n, fp) != n ||
            std::fwrite(degree.data(), sizeof(uint32_t), n, fp) != n || std::fwrite(kind.data(), sizeof(uint8_t), n, fp) != n)
            die("Error writing to binary file");
        if (o.has_stats) gs.write_binary(fp, n);
        return;
    }
    std::fprintf(fp, "#Cluster\t%s\t%s\t%.6g\tdbscan\t%u\t%s\n", kMeasureNames[o.result_type], is_distance(o.result_type) ? "<=" : ">=",
                 (double)o.cluster_t, o.min_pts, o.assign_mode == DSH_GREEDY_BEST ? "best" : "first");  // --threshold's number format
    std::vector<uint32_t> index(std::max<size_t>(n, 1));
    uint32_t next = 0;
    for (size_t x = 0; x < n; ++x)
        if (kind[x] == DSH_DBSCAN_CORE && labels[x] == x) index[x] = next++;
    static const char *const kKinds[3] = {"noise", "border", "core"};
    std::string s;
    char num[64];
    for (size_t x = 0; x < n; ++x) {
        s = names[x];
        if (kind[x] == DSH_DBSCAN_NOISE) s += "\t-\t-";
        else {
            s.append(num, (size_t)std::snprintf(num, sizeof num, "\t%u\t", index[labels[x]]));
            s += names[labels[x]];
        }
        s.append(num, (size_t)std::snprintf(num, sizeof num, "\t%s\t%u", kKinds[kind[x] <= DSH_DBSCAN_CORE ? kind[x] : 0], degree[x]));
        if (o.has_stats) gs.append_fields(s, x, names);
        s += '\n';
        std::fwrite(s.data(), 1, s.size(), fp);
    }
}

// --mst: the minimum spanning tree of the pair values (dsh_mst), or with --dendrogram its merge table (dsh_mst_linkage).  No
// pair leaves the device: n - 1 edges do
static void emit_mst(const DistRun &r, std::FILE *fp)
{
    const Opts &o = r.o;
    const size_t n = r.n;
    const std::vector<std::string> &names = o.inpaths;
    const float inf = std::numeric_limits<float>::infinity();
    const float cutoff = o.has_mst_cutoff ? o.mst_cutoff : (is_distance(o.result_type) ? inf : -inf);
    const size_t room = std::max<size_t>(n, 2) - 1;
    std::vector<uint32_t> lhs(room), rhs(room), size(room);
    std::vector<float> val(room);
    uint64_t m = 0;
    DSH(r.ctx, dsh_mst(r.ctx, o.estim, o.result_type, o.k, cutoff, lhs.data(), rhs.data(), val.data(), &m, nullptr));
    if (o.dendrogram) {  // (the values stay where they are: row s takes the value of edge s)
        std::vector<uint32_t> za(room), zb(room);
        if (dsh_mst_linkage(n, lhs.data(), rhs.data(), val.data(), m, za.data(), zb.data(), val.data(), size.data()) != DSH_OK)
            die("internal: the edges of dsh_mst are not a forest");
        lhs.swap(za), rhs.swap(zb);
    }
    if (o.fmt == BINARY) {
        const uint64_t hdr[2] = {(uint64_t)n, m};
        if (std::fwrite(hdr, sizeof(uint64_t), 2, fp) != 2 || std::fwrite(lhs.data(), sizeof(uint32_t), m, fp) != m ||
            std::fwrite(rhs.data(), sizeof(uint32_t), m, fp) != m || std::fwrite(val.data(), sizeof(float), m, fp) != m ||
            (o.dendrogram && std::fwrite(size.data(), sizeof(uint32_t), m, fp) != m))
            die("Error writing to binary file");
        return;
    }
    std::fprintf(fp, "#%s\t%s\t%zu\t%llu\n", o.dendrogram ? "Dendrogram" : "MST", kMeasureNames[o.result_type], n, (unsigned long long)m);
    for (size_t e = 0; e < m; ++e) {  // --representatives' number format
        if (o.dendrogram) std::fprintf(fp, "%u\t%u\t%.6g\t%u\n", lhs[e], rhs[e], (double)val[e], size[e]);
        else std::fprintf(fp, "%s\t%s\t%.6g\n", names[lhs[e]].c_str(), names[rhs[e]].c_str(), (double)val[e]);
    }
}

// --histogram: the distribution of the values (dsh_dist_histogram / dsh_dist_rect_histogram): only counts leave the device
static void emit_histogram(const DistRun &r, std::FILE *fp)
{
    const Opts &o = r.o;
    const size_t n = r.n, nq = r.nq;
    check_query_count(n, nq);
    const bool split = !o.hist_labels_file.empty();
    if (split && r.hist_labels.size() != n)
        die("--histogram-labels: %s labels %zu inputs but this run has %zu", o.hist_labels_file.c_str(), r.hist_labels.size(), n);
    const size_t ne = o.hist_edges.size(), nclass = ne + 2, planes = split ? 2 : 1;
    const uint32_t *lab = split ? r.hist_labels.data() : nullptr;
    std::vector<uint64_t> counts(planes * nclass);
    if (nq) DSH(r.ctx, dsh_dist_rect_histogram(r.ctx, o.estim, o.result_type, o.k, n - nq, n, 0, n - nq, o.hist_edges.data(), (uint32_t)ne, lab, counts.data()));
    else DSH(r.ctx, dsh_dist_histogram(r.ctx, o.estim, o.result_type, o.k, 0, n, o.hist_edges.data(), (uint32_t)ne, lab, counts.data()));
    if (o.fmt == BINARY) {
        const uint64_t hdr[2] = {(uint64_t)ne, (uint64_t)planes};
        const float pad = 0.f;
        if (std::fwrite(hdr, sizeof(uint64_t), 2, fp) != 2 || std::fwrite(o.hist_edges.data(), sizeof(float), ne, fp) != ne ||
            ((ne & 1) && std::fwrite(&pad, sizeof(float), 1, fp) != 1) ||
            std::fwrite(counts.data(), sizeof(uint64_t), counts.size(), fp) != counts.size())
            die("Error writing to binary file");
        return;
    }
    std::fprintf(fp, "#Histogram\t%s\t%s\n", kMeasureNames[o.result_type], is_distance(o.result_type) ? "<=" : ">=");
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    for (size_t b = 0; b < nclass; ++b) {  // --threshold's number format
        const double lo = b == ne + 1 ? nan : (b == 0 ? -inf : (double)o.hist_edges[b - 1]);
        const double hi = b == ne + 1 ? nan : (b == ne ? inf : (double)o.hist_edges[b]);
        std::fprintf(fp, "%.6g\t%.6g\t%llu", lo, hi, (unsigned long long)counts[b]);
        if (split) std::fprintf(fp, "\t%llu", (unsigned long long)counts[nclass + b]);
        std::fputc('\n', fp);
    }
}

// --union-curve: the size of the union of the first i + 1 inputs for every i (dsh_union_curve), and with --curve-permutations N
// the mean (summed in the permutations' order, divided once), minimum and maximum of every step over the N orders of
// dsh_curve_permutations(n, N, seed)
static void emit_union_curve(const DistRun &r, std::FILE *fp)
{
    static const char *const kEstimNames[3] = {"ORIGINAL", "ERTL_IMPROVED", "ERTL_MLE"};
    const Opts &o = r.o;
    const uint64_t n = r.n, N = o.curve_perms;
    std::vector<uint32_t> orders((1 + N) * n);
    for (uint64_t i = 0; i < n; ++i) orders[i] = (uint32_t)i;
    if (dsh_curve_permutations(n, N, o.curve_seed, orders.data() + n) != DSH_OK) die("--curve-permutations: %llu inputs are too many", (unsigned long long)n);
    std::vector<double> card((1 + N) * n);
    DSH(r.ctx, dsh_union_curve(r.ctx, o.estim, orders.data(), n, 1 + N, card.data(), nullptr));
    if (o.fmt == BINARY) {
        const uint64_t hdr[2] = {n, N};
        if (std::fwrite(hdr, sizeof(uint64_t), 2, fp) != 2 || std::fwrite(card.data(), sizeof(double), card.size(), fp) != card.size())
            die("Error writing to binary file");
        return;
    }
    std::fprintf(fp, "#UnionCurve\t%s\tpermutations=%llu\tseed=%llu\n", kEstimNames[o.estim], (unsigned long long)N, (unsigned long long)o.curve_seed);
    std::fprintf(fp, "#step\tname\tunion_size\tnew%s\n", N ? "\tperm_mean\tperm_min\tperm_max" : "");
    for (uint64_t i = 0; i < n; ++i) {
        std::fprintf(fp, "%llu\t%s\t%.3f\t%.3f", (unsigned long long)(i + 1), o.inpaths[i].c_str(), card[i], i ? card[i] - card[i - 1] : card[i]);
        if (N) {
            double sum = 0, lo = card[n + i], hi = card[n + i];
            for (uint64_t q = 0; q < N; ++q) {
                const double v = card[(1 + q) * n + i];
                sum += v, lo = std::min(lo, v), hi = std::max(hi, v);
            }
            std::fprintf(fp, "\t%.3f\t%.3f\t%.3f", sum / (double)N, lo, hi);
        }
        std::fputc('\n', fp);
    }
}

// --threshold: only the pairs that pass (dsh_dist_threshold / dsh_dist_rect_threshold): no dense matrix
static void emit_threshold(const DistRun &r, std::FILE *fp)
{
    const Opts &o = r.o;
    const size_t n = r.n, nq = r.nq;
    const std::vector<std::string> &names = o.inpaths;
    check_query_count(n, nq);
    const size_t nr = n - nq, rows = nq ? nq : n;
    std::vector<uint64_t> row_ptr(rows + 1);
    uint32_t *col = nullptr;
    float *val = nullptr;
    uint64_t nnz = 0;
    if (nq) DSH(r.ctx, dsh_dist_rect_threshold(r.ctx, o.estim, o.result_type, o.k, nr, n, 0, nr, o.threshold, row_ptr.data(), &col, &val, &nnz));
    else DSH(r.ctx, dsh_dist_threshold(r.ctx, o.estim, o.result_type, o.k, 0, n, o.threshold, row_ptr.data(), &col, &val, &nnz));
    if (o.fmt == BINARY) {
        const uint64_t hdr[2] = {(uint64_t)rows, nnz};
        if (std::fwrite(hdr, sizeof(uint64_t), 2, fp) != 2 || std::fwrite(row_ptr.data(), sizeof(uint64_t), rows + 1, fp) != rows + 1 ||
            std::fwrite(col, sizeof(uint32_t), nnz, fp) != nnz || std::fwrite(val, sizeof(float), nnz, fp) != nnz)
            die("Error writing to binary file");
    } else {
        std::fprintf(fp, "#Threshold\t%s\t%s\t%.6g\n", kMeasureNames[o.result_type], is_distance(o.result_type) ? "<=" : ">=", (double)o.threshold);
        std::string s;
        char num[64];
        for (size_t q = 0; q < rows; ++q) {
            s.clear();
            const std::string &name = names[nq ? nr + q : q];
            for (uint64_t h = row_ptr[q]; h < row_ptr[q + 1]; ++h) {
                s += name;
                s += '\t';
                s += names[col[h]];
                s.append(num, (size_t)std::snprintf(num, sizeof num, "\t%.6g\n", (double)val[h]));  // format_ut_row's number format
            }
            std::fwrite(s.data(), 1, s.size(), fp);
        }
    }
    dsh_free_host(col);
    dsh_free_host(val);
}

// --nearest-neighbors: nndist_loop (src/sketch_and_cmp.h:712-783)
static void emit_nearest_neighbors(const DistRun &r, std::FILE *fp)
{
    const Opts &o = r.o;
    const size_t n = r.n, nq = r.nq;
    const size_t nr = nq ? n - nq : n, npairs = nq ? nq : n;
    unsigned nn = o.nneighbors;
    const size_t possible = nq ? nr : (n ? n - 1 : 0);
    if (nn > possible) {
        std::fprintf(stderr, "Only reporting %zu rather than %u neighbors due to their being only that many sets.\n", possible, nn);
        nn = (unsigned)possible;
    }
    std::vector<uint32_t> idx(std::max<size_t>(npairs * nn, 1));
    std::vector<float> val(std::max<size_t>(npairs * nn, 1));
    if (nn) DSH(r.ctx, dsh_knn(r.ctx, o.estim, o.result_type, o.k, nq ? nr : 0, n, 0, nr, nn, idx.data(), val.data()));
    if (o.fmt == BINARY) {  // u32 n, u32 nn, then {float value, u32 id} pairs (validx_t, :605)
        uint32_t hdr[2] = {(uint32_t)n, nn};
        std::fwrite(hdr, sizeof(uint32_t), 2, fp);
        for (size_t t = 0; t < npairs * nn; ++t) {
            std::fwrite(&val[t], sizeof(float), 1, fp);
            std::fwrite(&idx[t], sizeof(uint32_t), 1, fp);
        }
    } else {  // rows in input order (the reference's row order depends on its thread schedule)
        std::fputs("#File\tNeighbor ID:distance\t...\n", fp);
        for (size_t i = 0; i < npairs; ++i) {
            std::string s(o.inpaths[i + (nq ? nr : 0)]);
            char num[64];
            for (unsigned j = 0; j < nn; ++j)
                s.append(num, (size_t)std::snprintf(num, sizeof num, "\t%u:%g", idx[i * nn + j], (double)val[i * nn + j]));
            s += '\n';
            std::fwrite(s.data(), 1, s.size(), fp);
        }
    }
}

// -Q, or an asymmetric measure: partdist_loop (src/dashing.h:660-712): one row per query over all references
static void emit_rectangle(const DistRun &r, std::FILE *fp)
{
    const Opts &o = r.o;
    const size_t n = r.n, nq = r.nq;
    check_query_count(n, nq);
    const size_t nr = n - nq;
    if (o.fmt == UPPER_TRIANGULAR) std::fprintf(fp, "%zu\n", n);  // src/sketch_and_cmp.h:394-396
    const size_t qblock = std::max<size_t>(1, ((size_t)64 << 20) / nr);
    std::vector<float> buf;
    for (size_t q0 = nr; q0 < n; q0 += qblock) {
        const size_t q1 = std::min(n, q0 + qblock);
        buf.resize((q1 - q0) * nr);
        DSH(r.ctx, dsh_dist_rect(r.ctx, o.estim, o.result_type, o.k, q0, q1, 0, nr, buf.data()));
        for (size_t qi = q0; qi < q1; ++qi) {
            const float *row = buf.data() + (qi - q0) * nr;
            if (o.fmt == BINARY) {
                if (std::fwrite(row, sizeof(float), nr, fp) != nr) die("Error writing to binary file");
            } else {
                std::string s(o.inpaths[qi]);
                char num[64];
                for (size_t j = 0; j < nr; ++j) s.append(num, (size_t)std::snprintf(num, sizeof num, "\t%g", (double)row[j]));
                s += '\n';
                std::fwrite(s.data(), 1, s.size(), fp);
            }
        }
    }
}

// -b to a file on several GPUs of one node: every device holds all sketches, device d computes the row range dsh_balance_rows
// gives it (tile-aligned, equal tile counts) and writes its contiguous span of the packed matrix straight into the output
// file, block by block at the block's offset
static void emit_multi_device_file(const DistRun &r, std::FILE *fp)
{
    const Opts &o = r.o;
    const size_t n = r.n;
    if (write_binary_header(fp, n)) die("Failure");
    std::fflush(fp);
    const int fd = ::fileno(fp);
    if (::ftruncate(fd, (off_t)(9 + tri_total(n) * sizeof(float)))) die("could not size %s", o.out_dists.c_str());
    const size_t G = o.devices.size();
    std::vector<uint8_t> all(n << o.S);
    DSH(r.ctx, dsh_download_sketches(r.ctx, 0, n, all.data()));
    std::vector<uint64_t> bounds(G + 1);
    if (dsh_balance_rows(n, (uint32_t)G, bounds.data())) die("dsh_balance_rows failed");
    std::vector<std::thread> workers;
    for (size_t d = 0; d < G; ++d)
        workers.emplace_back([&, d]() {
            dsh_ctx *c = d ? secondary_context(o.devices[d], all, n, o.S) : r.ctx;
            for_row_blocks(c, o, n, bounds[d], bounds[d + 1], r.block_vals, [&](uint64_t rb, uint64_t, const float *vals, uint64_t span) {
                const off_t pos = (off_t)(9 + dsh_tri_span(n, 0, rb) * sizeof(float));
                size_t done = 0;
                while (done < span * sizeof(float)) {
                    const ssize_t w = ::pwrite(fd, (const char *)vals + done, span * sizeof(float) - done, pos + (off_t)done);
                    if (w <= 0) die("Failed to write rows to disk");
                    done += (size_t)w;
                }
            });
            if (d > 0) dsh_destroy(c);
        });
    for (auto &w : workers) w.join();
}

// Several GPUs (or --rccl), output that one writer has to emit in order (text formats, or -b to a pipe): every device
// computes its rows -- the library partitions them itself (dsh_dist_collect with bounds = NULL: a row range per
// device plus top-up tile rows from the bottom of the triangle, dsh_balance_rowsets) -- and the rows are delivered
// to the first device over RCCL / xGMI inside the library (pipelined grouped ncclSend/ncclRecv, part by part),
// which hands the whole matrix to this process -- dashing's single writer (src/sketch_and_cmp.h:804-849) fed by
// G GPUs.  One thread per device, as RCCL wants for one process.
static void emit_rccl_collect(const DistRun &r, std::FILE *fp)
{
    const Opts &o = r.o;
    const size_t n = r.n;
    const uint64_t total = tri_total(n);
    const size_t G = std::max<size_t>(o.devices.size(), 1);
    uint8_t uid[DSH_UNIQUE_ID_BYTES];
    if (int rc = dsh_comm_unique_id(uid)) die("[dashing-amd] RCCL is not available (dsh_comm_unique_id = %d)", rc);
    std::vector<uint8_t> all;
    if (G > 1) {
        all.resize(n << o.S);
        DSH(r.ctx, dsh_download_sketches(r.ctx, 0, n, all.data()));
    }
    std::vector<float> tri(std::max<uint64_t>(total, 1));
    std::vector<std::thread> workers;
    for (size_t d = 0; d < G; ++d)
        workers.emplace_back([&, d]() {
            dsh_ctx *c = d ? secondary_context(o.devices[d], all, n, o.S) : r.ctx;
            DSH(c, dsh_comm_init(c, uid, (int)d, (int)G));
            DSH(c, dsh_dist_collect(c, o.estim, o.result_type, o.k, /*bounds=*/nullptr, 0, d == 0 ? tri.data() : nullptr));
            DSH(c, dsh_comm_destroy(c));
            if (d > 0) dsh_destroy(c);
        });
    for (auto &w : workers) w.join();
    if (o.fmt == BINARY) {
        if (write_binary_header(fp, n)) die("Failure");
        if (total && std::fwrite(tri.data(), sizeof(float), total, fp) != total) die("Failed to write rows to disk");
    } else if (o.fmt == FULL_TSV) {
        emit_full_header(fp, o.inpaths);
        for (size_t i = 0; i < n; ++i) emit_full_row(fp, o.inpaths, i, tri.data());
    } else {
        emit_header(fp, o.fmt, o.inpaths);
        for (size_t i = 0; i < n; ++i) emit_ut_row(fp, o.fmt, o.inpaths, i, tri.data() + dsh_tri_span(n, 0, i));
    }
}

// -T: the full table needs the whole triangle at once
static void emit_full_tsv(const DistRun &r, std::FILE *fp)
{
    const Opts &o = r.o;
    std::vector<float> tri(std::max<uint64_t>(tri_total(r.n), 1));
    DSH(r.ctx, dsh_dist_rows(r.ctx, o.estim, o.result_type, o.k, 0, r.n, tri.data()));
    emit_full_header(fp, o.inpaths);
    for (size_t i = 0; i < r.n; ++i) emit_full_row(fp, o.inpaths, i, tri.data());
}

// The streamed triangle (dist_loop, src/sketch_and_cmp.h:785-880), -b or one text line per row: a block is written, or its rows
// formatted on all host threads, while the device computes the next one
static void emit_triangle(const DistRun &r, std::FILE *fp)
{
    const Opts &o = r.o;
    const uint64_t n = r.n;
    if (o.fmt == BINARY) {
        if (write_binary_header(fp, n)) die("Failure");
    } else {
        emit_header(fp, o.fmt, o.inpaths);
    }
    for_row_blocks(r.ctx, o, n, 0, n, r.block_vals, [&](uint64_t rb, uint64_t re, const float *buf, uint64_t span) {
        if (o.fmt == BINARY) {
            if (span && std::fwrite(buf, sizeof(float), span, fp) != span) die("Failed to write rows to disk");
            return;
        }
        // format rows on all host threads (snprintf dominates text output), write in order
        std::vector<uint64_t> off(re - rb + 1, 0);
        for (uint64_t i = rb; i < re; ++i) off[i - rb + 1] = off[i - rb] + (n - i - 1);
        const uint64_t group = 64;
        for (uint64_t g0 = rb; g0 < re; g0 += group * (uint64_t)o.nthreads) {
            const uint64_t g1 = std::min<uint64_t>(re, g0 + group * (uint64_t)o.nthreads);
            std::vector<std::string> rows(g1 - g0);
#pragma omp parallel for schedule(dynamic, 4) num_threads(o.nthreads)
            for (int64_t i = (int64_t)g0; i < (int64_t)g1; ++i)
                format_ut_row(rows[i - g0], o.fmt, o.inpaths, (size_t)i, buf + off[i - rb]);
            for (auto &row : rows) std::fwrite(row.data(), 1, row.size(), fp);
        }
    });
}

static int dist_main(int argc, char **argv, bool by_seq = false)
{
    DistRun r;
    Opts &o = r.o;
    o = parse(argc, argv, true);
    r.block_vals = block_vals_from_env();
    if (by_seq) o.avoid_sorting = 1;  // records keep their order
    refuse_conflicts(o, by_seq);
    if (!o.pairs_file.empty()) r.pair_types = parse_measures(o);
    if (by_seq) read_records_or_presketched(r);
    read_option_files(r);
    std::FILE *ofp = stdout, *pairofp = stdout;
    if (!o.out_sizes.empty() && !(ofp = std::fopen(o.out_sizes.c_str(), "w"))) die("Could not open file at %s for writing.", o.out_sizes.c_str());
    if (!o.out_dists.empty() && !(pairofp = std::fopen(o.out_dists.c_str(), "wb"))) die("Could not open file at %s for writing.", o.out_dists.c_str());
    order_paths(r);
    if (!o.groups_file.empty()) parse_groups_file(r);
    if (!o.pairs_file.empty()) look_up_pairs(r);

    const double t_start = now_s();
    since_launch("dist: options parsed, context thread about to start");
    CtxFuture cf(o.device, r.n, o.S, (o.presketched || by_seq) ? 0 : staging_bytes_for(o.inpaths));  // the HIP runtime comes up while the first batch is read
    const double t_fill0 = now_s();
    if (by_seq) load_records(cf.get(), r);
    else if (o.presketched) load_hll_files(cf.get(), o, r.n);
    else fill_sketches(cf, o, /*write_files=*/o.cache != 0, false);
    r.ctx = cf.get();
    if (g_timing) std::fprintf(stderr, "[timing] all sketches resident after %.3f s\n", now_s() - t_fill0);
    if (!o.groups_file.empty()) union_groups(r);
    write_sizes(r, ofp);

    if (!o.pairs_file.empty()) emit_pairs(r, pairofp);
    else if (o.has_cluster && o.has_min_pts) emit_dbscan(r, pairofp);
    else if (o.has_cluster || o.has_reps) emit_labelling(r, pairofp);
    else if (o.has_hist) emit_histogram(r, pairofp);
    else if (o.has_curve) emit_union_curve(r, pairofp);
    else if (o.has_mst) emit_mst(r, pairofp);
    else if (o.has_threshold) emit_threshold(r, pairofp);
    else if (o.nneighbors) emit_nearest_neighbors(r, pairofp);
    else if (r.nq) emit_rectangle(r, pairofp);
    else if (o.fmt == BINARY && o.devices.size() > 1 && !o.out_dists.empty()) emit_multi_device_file(r, pairofp);
    else if (o.devices.size() > 1 || o.rccl) emit_rccl_collect(r, pairofp);
    else if (o.fmt == FULL_TSV) emit_full_tsv(r, pairofp);
    else emit_triangle(r, pairofp);

    std::fflush(pairofp);
    if (pairofp != stdout) std::fclose(pairofp);
    if (g_timing) std::fprintf(stderr, "[timing] total since dsh_create %.3f s\n", now_s() - t_start);
    if (o.fmt == BINARY && !o.nneighbors) {  // src/distmain.cpp:191-200 (emit_fmt == BINARY exactly)
        const std::string labels = o.out_dists.empty() ? "unspecified" : o.out_dists + ".labels";
        if (write_labels(labels, o.inpaths)) die("Could not open file at '%s' for writing", labels.c_str());
    }
    leave(r.ctx);
    return EXIT_SUCCESS;
}

int main(int argc, char **argv)
{
    // (Round 2 called setenv("OMP_WAIT_POLICY", "passive") here; libgomp reads its environment in a constructor that runs
    // before main(), so that never took effect -- ADVICE r2 -- and a re-exec with the variable set costs more process
    // start-up than the few milliseconds idle workers spin by default.  Set OMP_WAIT_POLICY=passive in the environment
    // if the host threads are needed elsewhere between the parallel regions.)
    since_launch("main() entered");
    if (argc < 2 || !std::strcmp(argv[1], "-h") || !std::strcmp(argv[1], "--help")) {
        std::fprintf(stderr, "%s\nUsage: dashing-amd <subcommand> [options...]\nSubcommands:\n  sketch\n  dist (also: cmp, setdist)\n  sketch_by_seq | dist_by_seq   (one sketch per sequence record)\n  union | fold | view   (utilities on .hll files)\n  printmat              (binary distance matrix -> text)\n  hll                   (cardinality of the k-mers of a set of files)\n", kVersion);
        return EXIT_FAILURE;
    }
    const std::string sub(argv[1]);
    if (sub == "sketch") return sketch_main(argc - 1, argv + 1);
    if (sub == "dist" || sub == "cmp" || sub == "setdist") return dist_main(argc - 1, argv + 1);
    if (sub == "sketch_by_seq") return sketch_by_seq_main(argc - 1, argv + 1);
    if (sub == "dist_by_seq") return dist_main(argc - 1, argv + 1, /*by_seq=*/true);
    if (sub == "union") return union_main(argc - 1, argv + 1);
    if (sub == "view") return view_main(argc - 1, argv + 1);
    if (sub == "fold") return fold_main(argc - 1, argv + 1);
    if (sub == "hll") return hll_main(argc - 1, argv + 1);
    if (sub == "printmat") return printmat_main(argc - 1, argv + 1);
    if (sub == "version" || sub == "--version") {
        std::printf("%s\nbackend: %s\n", kVersion, dsh_backend_name());
        return EXIT_SUCCESS;
    }
    std::fprintf(stderr, "subcommand '%s' is outside the HLL sketch+dist hot path this build covers\n", sub.c_str());
    return EXIT_FAILURE;
}
