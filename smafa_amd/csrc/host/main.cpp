// main.cpp — the `smafa` command line over libsmafa_amd.so.  Subcommands, flag names and value types
// follow the reference's clap tree (/root/reference/src/main.rs:64-116):
//   makedb  -i/--input FILE  -d/--database FILE
//   query   -d/--database FILE  -q/--query FILE  [--max-divergence INT] [--max-num-hits INT]
//           [--limit-per-sequence INT]
//   cluster -i/--input FILE  -d/--max-divergence INT
//   count   -i/--input FILE...
//   pairs   -d/--database FILE  --max-divergence INT  [--since ROW]   (this build only: every pair of the DB's own subjects
//           within the bound; --since: those whose larger sequence number is at least ROW)
//   components -d/--database FILE  --max-divergence INT  [--levels]   (this build only: the single-linkage component of
//           every subject; --levels: at every bound 0 .. INT)
//   forest  -d/--database FILE  --max-divergence INT  [--min-pts INT [--cores]]   (this build only: the minimum spanning forest
//           of the subjects up to the bound, the merge tree of the components at every bound 0 .. INT; --min-pts: the forest
//           under the mutual-reachability distance, the merge tree of the density clusters; --cores: the core distances instead)
//   stable  -d/--database FILE  --max-divergence INT  --min-pts INT  [--min-cluster-size INT] [--joined]   (this build only: the
//           stable cluster of every subject, HDBSCAN's selection over the forest under the mutual-reachability distance)
//   consensus -d/--database FILE  --labels FILE|-   (this build only: per cluster of a labels file, as components, density, peaks
//           and stable print them, its size, the member nearest to its consensus, the greatest divergence from it, and the consensus)
//   density -d/--database FILE  --max-divergence INT  --min-pts INT   (this build only: the density cluster (DBSCAN) and the
//           number of neighbours within the bound of every subject)
//   peaks   -d/--database FILE  --max-divergence INT  [--radius INT] [--sizes FILE|-]   (this build only: the abundance-peak cluster,
//           the parent and the weight of every subject; --sizes: the weights of a file, the sizes of dereplicated sequences, summed)
//   chimeras -d/--database FILE  --max-divergence INT  [--min-fold INT] [--radius INT] [--weights FILE|-]   (this build only: the
//           chimera check, per subject its flag, its best left and right parent with the shared prefix / suffix length, its weight)
//   table   -d/--database FILE  -q/--query FILE  --max-divergence INT  [--labels FILE|-] [--samples FILE|-] [--weights FILE|-]
//           [--per-read | --per-sequence]   (this build only: the reads assigned to their nearest subject within the bound and
//           counted per (label, sample); or per read its subject and distance; or per subject its count)
//   classify -d/--database FILE  -q/--query FILE  --max-divergence INT  --taxonomy FILE|-  [--slack INT] [--samples FILE|-]
//           [--weights FILE|-] [--per-read]   (this build only: the reads given the lowest common ancestor of the lineages of their
//           best hits and counted per (taxon, sample); or per read its anchor, distance, ties, depth and lineage)
//   neighbours -d/--database FILE  --max-divergence INT  [--max-num-hits INT]   (this build only: per subject its neighbours
//           within the bound, nearest first)
//   subset  -d/--database FILE  (--keep FILE|- | --drop FILE|-)  --output FILE   (this build only: the listed sequences, or all but
//           them, as a packed store of their own; "new<TAB>old" per kept sequence)
// plus -v/--verbose and --quiet (logging only; results are the only thing on stdout).
// Additions of this build: --device N (query, cluster), --gpus N (query, cluster: GPUs 0..N-1, one handle and host thread
// each; the output does not depend on N), --devices a,b,.. (query, cluster: explicit list, entries may repeat),
// --alphabet nt|aa (makedb, cluster), --packed (makedb: the packed store file, host/packed.cpp).
// Exit status: 0 ok, 101 where the reference panics (a Rust panic exits 101), 1 other failures, 2 usage.
#include <cerrno>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <time.h>
#include <unistd.h>

#include <string>
#include <vector>

#include "../../../include/smafa_amd.h"

static int usage(const char *msg, FILE *to = stderr) {
    if (msg) fprintf(stderr, "error: %s\n\n", msg);
    fprintf(to,
            "Usage: smafa <COMMAND>\n\n"
            "Commands:\n"
            "  makedb   Generate a searchable database\n"
            "  query    Search a database. See query --help for more information about output format.\n"
            "  cluster  Cluster sequences by similarity\n"
            "  count    Print the number of reads/bases in a possibly gzipped FASTX file\n\n"
            "makedb  -i, --input <FILE>  -d, --database <FILE>  [--alphabet nt|aa] [--packed [--device <N>]]\n"
            "        --packed: write the store as it lies in GPU memory (loads without decoding); packed on the GPU, or by\n"
            "        host threads when there is none or with --no-gpu (the same bytes)\n"
            "query   -d, --database <FILE>  -q, --query <FILE>  [--max-divergence <INT>] [--max-num-hits <INT>]\n"
            "        [--limit-per-sequence <INT>] [--device <N> | --gpus <N> | --devices <a,b,..>]\n"
            "        Output columns (tab-separated): query number (0-indexed), subject number (0-indexed),\n"
            "        divergence, subject sequence (dashes and degenerate bases shown as N)\n"
            "cluster -i, --input <FILE>  -d, --max-divergence <INT>  [--alphabet nt|aa] [--device <N> | --gpus <N> | --devices <a,b,..>]\n"
            "count   -i, --input <FILE>...\n"
            "pairs   -d, --database <FILE>  --max-divergence <INT>  [--device <N>]  (not in the reference: every pair i < j of the\n"
            "        database's own sequences within the bound, one \"i<TAB>j<TAB>divergence\" line each)\n"
            "        [--since <ROW>]: only the pairs with j >= ROW, the pairs that the sequences from number ROW on have added\n"
            "components -d, --database <FILE>  --max-divergence <INT>  [--levels] [--device <N>]  (not in the reference: single-linkage\n"
            "        components of the database's own sequences at the bound, one \"i<TAB>label\" line per sequence, label = the\n"
            "        smallest sequence number of its component; --levels: one label column per bound 0 .. <INT>,\n"
            "        \"i<TAB>label_0<TAB>...<TAB>label_INT\", from one join)\n"
            "forest  -d, --database <FILE>  --max-divergence <INT>  [--min-pts <INT> [--cores]]  [--device <N>]  (not in the reference: a minimum spanning forest of\n"
            "        the database's own sequences under the pairs within the bound, one \"a<TAB>b<TAB>divergence\" line per edge, a < b,\n"
            "        ordered by divergence, then a, then b; the lines up to divergence t are the merge tree of `components` at t;\n"
            "        which of several pairs of equal divergence joins two components may differ from run to run)\n"
            "        [--min-pts <INT>]: the forest under the mutual-reachability distance max(divergence, core(a), core(b)) in the\n"
            "        third column, core(i) = the divergence of sequence i's (min-pts - 1)-th nearest other sequence; the lines up to\n"
            "        weight t are the merge tree of the core sequences of `density` at bound t; sequences with fewer than min-pts - 1\n"
            "        others within the bound are in no line; --cores: one \"i<TAB>core\" line per sequence instead, -1 for those)\n"
            "stable  -d, --database <FILE>  --max-divergence <INT>  --min-pts <INT>  [--min-cluster-size <INT>] [--joined]  [--device <N>]\n"
            "        (not in the reference: stable clusters of the database's own sequences, one \"i<TAB>label\" line per sequence: the\n"
            "        clusters of `forest --min-pts` at every weight 0 .. <INT>, each kept at the levels where it persists longest (HDBSCAN's\n"
            "        excess of mass, counted in levels); label = the smallest sequence number of the cluster, -1 for noise; a cluster holds at\n"
            "        least min-cluster-size sequences (default: min-pts); --joined: a third column, the level at which the sequence joined)\n"
            "consensus -d, --database <FILE>  --labels <FILE|->  [--device <N>]  (not in the reference: one line per cluster of a labels\n"
            "        file, \"label<TAB>size<TAB>nearest<TAB>max_div<TAB>SEQUENCE\" in ascending label order; the file holds one\n"
            "        \"i<TAB>label\" line per sequence as `components`, `density`, `peaks` and `stable` print them (further columns are\n"
            "        ignored, -1: in no cluster, -: stdin); SEQUENCE = per column the letter most members hold, ties to the first of\n"
            "        A C G T N (amino acids: in code order); nearest = the member with the fewest differences from it, ties to the\n"
            "        smaller number; max_div = the most differences of any member:  smafa stable ... | smafa consensus -d DB --labels -)\n"
            "density -d, --database <FILE>  --max-divergence <INT>  --min-pts <INT>  [--device <N>]  (not in the reference: density\n"
            "        clusters (DBSCAN) of the database's own sequences, one \"i<TAB>label<TAB>degree\" line per sequence; degree = the\n"
            "        number of other sequences within the bound; a sequence is core if degree + 1 >= min-pts; label = the smallest\n"
            "        core sequence number of its cluster, for a non-core sequence that of its smallest core neighbour, -1 for noise)\n"
            "peaks   -d, --database <FILE>  --max-divergence <INT>  [--radius <INT>] [--sizes <FILE|->]  [--device <N>]  (not in the reference: abundance-peak\n"
            "        clusters of the database's own sequences, one \"i<TAB>label<TAB>parent<TAB>weight\" line per sequence; weight = 1 +\n"
            "        the number of other sequences within the radius (default 0: the number of exact copies); parent = the heaviest\n"
            "        sequence within the bound, ties to the smaller number, the sequence itself if none outranks it (a peak);\n"
            "        label = the peak reached by following the parents; --sizes: \"i<TAB>weight\" lines in any order, the sizes of\n"
            "        sequences that were dereplicated (further columns are ignored, a sequence without a line weighs 0, -: stdin):\n"
            "        weight = the sequence's own weight + those of the other sequences within the radius)\n"
            "chimeras -d, --database <FILE>  --max-divergence <INT>  [--min-fold <INT>] [--radius <INT>] [--weights <FILE|->]  [--device <N>]\n"
            "        (not in the reference: two-parent chimeras among the database's own sequences, one\n"
            "        \"i<TAB>flag<TAB>left_parent<TAB>left_len<TAB>right_parent<TAB>right_len<TAB>weight\" line per sequence; a parent is a\n"
            "        sequence within the bound that is heavier, and at least min-fold (default 2) times as heavy; left_parent shares the\n"
            "        longest prefix (left_len columns) with the sequence, right_parent the longest suffix, ties to the smaller number, -1\n"
            "        for none; flag = 1 where left_len + right_len covers the sequence: it is left_parent's head on right_parent's tail;\n"
            "        weight as in `peaks` (--radius, default 0: the number of exact copies), or from --weights, \"i<TAB>weight\" lines in any\n"
            "        order (further columns are ignored, a sequence without a line has weight 0 and takes no part, -: stdin); the bound\n"
            "        has to be at least the divergence of the parents one wants to catch)\n"
            "table   -d, --database <FILE>  -q, --query <FILE>  --max-divergence <INT>  [--labels <FILE|->] [--samples <FILE|->]\n"
            "        [--weights <FILE|->] [--per-read | --per-sequence]  [--device <N>]  (not in the reference: the abundance table; every\n"
            "        read of the query file is assigned to the database sequence with the fewest differences within the bound, ties to\n"
            "        the smaller number, and counted: one \"label<TAB>sample<TAB>count\" line per (label, sample) with a read, ordered by\n"
            "        label, then sample; the label of a read without a sequence within the bound is -1; --labels: a file as for\n"
            "        `consensus` (a sequence without a line: -1), default: every sequence is its own label; --samples, --weights:\n"
            "        \"read<TAB>value\" lines in any order, a read without a line is in sample 0 / weighs 1; at most one file is - (stdin);\n"
            "        --per-read: \"read<TAB>subject<TAB>divergence\" lines instead, -1 -1 for a read without a sequence; --per-sequence:\n"
            "        \"i<TAB>count\" lines, the weight assigned to each sequence:  smafa table ... --per-sequence | smafa chimeras ... --weights -)\n"
            "classify -d, --database <FILE>  -q, --query <FILE>  --max-divergence <INT>  --taxonomy <FILE|->  [--slack <INT>]\n"
            "        [--samples <FILE|->] [--weights <FILE|->] [--per-read]  [--device <N>]  (not in the reference: what SingleM does with\n"
            "        the rows of `query`; every read of the query file takes the lowest common ancestor of the lineages of its best hits —\n"
            "        the database sequences within its fewest differences + slack (default 0), all within the bound — and is counted: one\n"
            "        \"lineage<TAB>sample<TAB>count\" line per (taxon, sample) with a read, the lineage the names joined by ; down to the\n"
            "        node, \"root\" where the hits share no rank, \"unassigned\" for a read without a sequence within the bound; --taxonomy:\n"
            "        \"i<TAB>name;name;...\" lines in any order, most general name first, at most 16, blanks around a name are dropped,\n"
            "        further columns are ignored, a sequence without a line has no lineage; --samples, --weights: as for `table`; at most\n"
            "        one file is - (stdin); --per-read: \"read<TAB>subject<TAB>divergence<TAB>ties<TAB>depth<TAB>lineage\" lines instead,\n"
            "        -1 for subject, divergence and depth of a read without a sequence)\n"
            "neighbours -d, --database <FILE>  --max-divergence <INT>  [--max-num-hits <INT>]  [--device <N>]  (not in the reference: the\n"
            "        neighbour lists of the database's own sequences, one \"i<TAB>j<TAB>divergence\" line per sequence i and neighbour j\n"
            "        within the bound, both directions of every pair, ordered by i, then divergence, then j; --max-num-hits: at most\n"
            "        that many lines per i, the nearest, ties to the smaller j)\n"
            "subset  -d, --database <FILE>  (--keep <FILE|-> | --drop <FILE|->)  --output <FILE>  [--device <N>]  (not in the reference: the\n"
            "        listed sequences of the database, or all but the listed ones, written to --output as a packed store that every\n"
            "        command reads, renumbered in their old order; one \"new<TAB>old\" line per kept sequence; the list holds one sequence\n"
            "        number per line in its first column (further columns are ignored, repeats allowed, -: stdin):\n"
            "        smafa chimeras ... | awk '$2 == 1' | smafa subset -d DB --drop - --output CLEAN.db)\n");
    return 2;
}

static bool parse_u32(const char *s, uint32_t *out) {
    if (!s || !*s || *s == '-' || *s == '+') return false;
    char *end = nullptr;
    const unsigned long long v = strtoull(s, &end, 10);
    if (*end || v > 0xffffffffull) return false;
    *out = (uint32_t)v;
    return true;
}

static double wall_now() {
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec;
}

int main(int argc, char **argv) {
    const double t_main = wall_now();
    // top-level -v/--verbose and -q/--quiet in front of the subcommand (src/main.rs:67-68); the reference takes its log level
    // from the subcommand's own flags (set_log_level(m, true), :17,34,40,47), so these are accepted and change nothing
    int first = 1;
    while (first < argc && (!strcmp(argv[first], "-v") || !strcmp(argv[first], "--verbose") || !strcmp(argv[first], "-q") ||
                            !strcmp(argv[first], "--quiet")))
        first++;
    if (first >= argc) {  // no subcommand: the help text on stdout, and success (src/main.rs:52-56)
        usage(nullptr, stdout);
        printf("\n");
        return 0;
    }
    const std::string cmd = argv[first];
    if (cmd == "-h" || cmd == "--help") {
        usage(nullptr, stdout);
        return 0;
    }
    const bool is_cluster = cmd == "cluster";
    const char *input = nullptr, *database = nullptr, *query = nullptr, *labels = nullptr, *weights = nullptr, *samples = nullptr, *taxonomy = nullptr, *keep = nullptr, *drop = nullptr, *output = nullptr, *sizes = nullptr;
    std::vector<const char *> count_paths;
    uint32_t max_div = SMAFA_NONE, max_hits = SMAFA_NONE, limit = SMAFA_NONE, device = 0, min_pts = 0, radius = 0, min_cluster_size = 0, min_fold = 2, slack = 0;
    bool have_min_pts = false, have_since = false;
    unsigned long long since = 0;
    bool have_max_div = false, packed = false, no_gpu = false, levels = false, cores = false, joined = false, per_read = false, per_sequence = false;
    std::vector<int> devices;  // query: more than one handle
    int alphabet = SMAFA_ALPHABET_NT;
    int verbosity = 1;  // the reference logs at info level unless told otherwise (bird_tool_utils set_log_level)
    if (const char *e = getenv("SMAFA_LOG")) verbosity = atoi(e);
    for (int i = first + 1; i < argc; i++) {
        const std::string a = argv[i];
        auto value = [&]() -> const char * { return i + 1 < argc ? argv[++i] : nullptr; };
        if (a == "-i" || a == "--input") {
            if (cmd == "count") {
                while (i + 1 < argc && argv[i + 1][0] != '-') count_paths.push_back(argv[++i]);
            } else if (!(input = value())) {
                return usage("--input needs a value");
            }
        } else if (a == "--database" || (a == "-d" && !is_cluster)) {
            if (!(database = value())) return usage("--database needs a value");
        } else if (a == "--max-divergence" || (a == "-d" && is_cluster)) {
            if (!parse_u32(value(), &max_div)) return usage("--max-divergence needs an unsigned integer");
            have_max_div = true;
        } else if (a == "-q" || a == "--query") {
            if (cmd == "query" || cmd == "table" || cmd == "classify") {
                if (!(query = value())) return usage("--query needs a value");
            } else {
                verbosity = 0;  // elsewhere -q is --quiet
            }
        } else if (a == "--max-num-hits") {
            if (!parse_u32(value(), &max_hits)) return usage("--max-num-hits needs an unsigned integer");
        } else if (a == "--limit-per-sequence") {
            if (!parse_u32(value(), &limit)) return usage("--limit-per-sequence needs an unsigned integer");
        } else if (a == "--device") {
            if (!parse_u32(value(), &device)) return usage("--device needs an unsigned integer");
        } else if (a == "--packed") {
            packed = true;
        } else if (a == "--min-pts" && (cmd == "density" || cmd == "forest" || cmd == "stable")) {
            if (!parse_u32(value(), &min_pts)) return usage("--min-pts needs an unsigned integer");
            have_min_pts = true;
        } else if (a == "--min-cluster-size" && cmd == "stable") {
            if (!parse_u32(value(), &min_cluster_size)) return usage("--min-cluster-size needs an unsigned integer");
        } else if (a == "--joined" && cmd == "stable") {
            joined = true;
        } else if (a == "--labels" && (cmd == "consensus" || cmd == "table")) {
            if (!(labels = value())) return usage("--labels needs a file, or - for stdin");
        } else if (a == "--radius" && (cmd == "peaks" || cmd == "chimeras")) {
            if (!parse_u32(value(), &radius)) return usage("--radius needs an unsigned integer");
        } else if (a == "--min-fold" && cmd == "chimeras") {
            if (!parse_u32(value(), &min_fold) || min_fold == 0) return usage("--min-fold needs a positive integer");
        } else if (a == "--weights" && (cmd == "chimeras" || cmd == "table" || cmd == "classify")) {
            if (!(weights = value())) return usage("--weights needs a file, or - for stdin");
        } else if (a == "--samples" && (cmd == "table" || cmd == "classify")) {
            if (!(samples = value())) return usage("--samples needs a file, or - for stdin");
        } else if (a == "--per-read" && (cmd == "table" || cmd == "classify")) {
            per_read = true;
        } else if (a == "--taxonomy" && cmd == "classify") {
            if (!(taxonomy = value())) return usage("--taxonomy needs a file, or - for stdin");
        } else if (a == "--slack" && cmd == "classify") {
            if (!parse_u32(value(), &slack)) return usage("--slack needs an unsigned integer");
        } else if (a == "--per-sequence" && cmd == "table") {
            per_sequence = true;
        } else if (a == "--keep" && cmd == "subset") {
            if (!(keep = value())) return usage("--keep needs a file, or - for stdin");
        } else if (a == "--drop" && cmd == "subset") {
            if (!(drop = value())) return usage("--drop needs a file, or - for stdin");
        } else if (a == "--sizes" && cmd == "peaks") {
            if (!(sizes = value())) return usage("--sizes needs a file, or - for stdin");
        } else if (a == "--output" && cmd == "subset") {
            if (!(output = value())) return usage("--output needs a value");
        } else if (a == "--since" && cmd == "pairs") {
            const char *v = value();
            char *end = nullptr;
            if (!v || !*v || *v == '-' || *v == '+') return usage("--since needs an unsigned integer");
            errno = 0;
            since = strtoull(v, &end, 10);
            if (*end || errno == ERANGE) return usage("--since needs an unsigned integer");
            have_since = true;
        } else if (a == "--levels" && cmd == "components") {
            levels = true;
        } else if (a == "--cores" && cmd == "forest") {
            cores = true;
        } else if (a == "--no-gpu") {
            no_gpu = true;
        } else if (a == "--gpus") {
            uint32_t g = 0;
            if (!parse_u32(value(), &g) || g < 1 || g > 64) return usage("--gpus needs a count between 1 and 64");
            devices.clear();
            for (uint32_t d = 0; d < g; d++) devices.push_back((int)d);
        } else if (a == "--devices") {
            const char *v = value();
            if (!v) return usage("--devices needs a comma-separated list");
            devices.clear();
            std::string tok;
            for (const char *c = v;; c++) {
                if (*c == ',' || *c == 0) {
                    uint32_t d = 0;
                    if (!parse_u32(tok.c_str(), &d)) return usage("--devices needs a comma-separated list of GPU ordinals");
                    devices.push_back((int)d);
                    tok.clear();
                    if (*c == 0) break;
                } else {
                    tok.push_back(*c);
                }
            }
        } else if (a == "--alphabet") {
            const char *v = value();
            if (v && !strcmp(v, "nt")) alphabet = SMAFA_ALPHABET_NT;
            else if (v && !strcmp(v, "aa")) alphabet = SMAFA_ALPHABET_AA;
            else return usage("--alphabet is nt or aa");
        } else if (a == "-v" || a == "--verbose") {
            verbosity = 2;  // debug
        } else if (a == "--quiet") {
            verbosity = 0;  // errors only
        } else if (a == "-h" || a == "--help") {
            usage(nullptr, stdout);
            return 0;
        } else {
            return usage(("unexpected argument " + a).c_str());
        }
    }
    smafa_set_verbosity(verbosity);
    int rc;
    if (cmd == "makedb") {
        if (!input || !database) return usage("makedb needs --input and --database");
        rc = packed ? smafa_makedb_packed(input, database, alphabet, no_gpu ? -1 : (int)device) : smafa_makedb(input, database, alphabet);
    } else if (cmd == "query") {
        if (!database || !query) return usage("query needs --database and --query");
        if (devices.empty()) devices.push_back((int)device);
        rc = smafa_query_multi(database, query, max_div, max_hits, limit, 1, devices.data(), (int)devices.size());
    } else if (is_cluster) {
        if (!input) return usage("cluster needs --input");
        if (!have_max_div) {  // src/main.rs:43 unwraps the option
            fprintf(stderr, "called `Option::unwrap()` on a `None` value\n");
            return 101;
        }
        if (devices.empty()) devices.push_back((int)device);
        rc = smafa_cluster_multi(input, max_div, 1, devices.data(), (int)devices.size(), alphabet);
    } else if (cmd == "pairs") {
        if (!database) return usage("pairs needs --database");
        if (!have_max_div) return usage("pairs needs --max-divergence");
        rc = have_since ? smafa_pairs_since(database, since, max_div, 1, (int)device) : smafa_pairs(database, max_div, 1, (int)device);
    } else if (cmd == "components") {
        if (!database) return usage("components needs --database");
        if (!have_max_div) return usage("components needs --max-divergence");
        rc = levels ? smafa_component_levels(database, max_div, 1, (int)device) : smafa_components(database, max_div, 1, (int)device);
    } else if (cmd == "forest") {
        if (!database) return usage("forest needs --database");
        if (!have_max_div) return usage("forest needs --max-divergence");
        if (cores && !have_min_pts) return usage("--cores needs --min-pts");
        rc = have_min_pts ? smafa_reach_forest(database, max_div, min_pts, cores ? 1 : 0, 1, (int)device)
                          : smafa_forest(database, max_div, 1, (int)device);
    } else if (cmd == "stable") {
        if (!database) return usage("stable needs --database");
        if (!have_max_div) return usage("stable needs --max-divergence");
        if (!have_min_pts) return usage("stable needs --min-pts");
        rc = smafa_stable(database, max_div, min_pts, min_cluster_size, joined ? 1 : 0, 1, (int)device);
    } else if (cmd == "consensus") {
        if (!database) return usage("consensus needs --database");
        if (!labels) return usage("consensus needs --labels");
        rc = smafa_consensus(database, labels, 1, (int)device);
    } else if (cmd == "density") {
        if (!database) return usage("density needs --database");
        if (!have_max_div) return usage("density needs --max-divergence");
        if (!have_min_pts) return usage("density needs --min-pts");
        rc = smafa_density(database, max_div, min_pts, 1, (int)device);
    } else if (cmd == "peaks") {
        if (!database) return usage("peaks needs --database");
        if (!have_max_div) return usage("peaks needs --max-divergence");
        rc = sizes ? smafa_peaks_weighted(database, max_div, radius, sizes, 1, (int)device) : smafa_peaks(database, max_div, radius, 1, (int)device);
    } else if (cmd == "chimeras") {
        if (!database) return usage("chimeras needs --database");
        if (!have_max_div) return usage("chimeras needs --max-divergence");
        rc = smafa_chimeras(database, max_div, radius, min_fold, weights, 1, (int)device);
    } else if (cmd == "table") {
        if (!database || !query) return usage("table needs --database and --query");
        if (!have_max_div) return usage("table needs --max-divergence");
        if (per_read && per_sequence) return usage("--per-read and --per-sequence exclude each other");
        rc = smafa_table(database, query, max_div, labels, samples, weights, per_read ? 1 : 0, per_sequence ? 1 : 0, 1, (int)device);
    } else if (cmd == "classify") {
        if (!database || !query) return usage("classify needs --database and --query");
        if (!have_max_div) return usage("classify needs --max-divergence");
        if (!taxonomy) return usage("classify needs --taxonomy");
        rc = smafa_classify(database, query, max_div, slack, taxonomy, samples, weights, per_read ? 1 : 0, 1, (int)device);
    } else if (cmd == "neighbours") {
        if (!database) return usage("neighbours needs --database");
        if (!have_max_div) return usage("neighbours needs --max-divergence");
        if (max_hits == 0) return usage("--max-num-hits needs a positive integer");
        rc = smafa_neighbours(database, max_div, max_hits, 1, (int)device);
    } else if (cmd == "subset") {
        if (!database || !output) return usage("subset needs --database and --output");
        if (keep && drop) return usage("--keep and --drop exclude each other");
        if (!keep && !drop) return usage("subset needs --keep or --drop");
        rc = smafa_subset(database, keep, drop, output, 1, (int)device);
    } else if (cmd == "count") {
        if (count_paths.empty()) return usage("count needs --input");
        rc = smafa_count(count_paths.data(), count_paths.size(), 1);
    } else {
        return usage(("unrecognized subcommand " + cmd).c_str());
    }
    if (verbosity >= 2) fprintf(stderr, "[DEBUG smafa] %s: %.3f s inside main()\n", cmd.c_str(), wall_now() - t_main);
    int code = 0;
    if (rc != SMAFA_OK) {
        fprintf(stderr, "%s\n", smafa_last_error());
        code = rc == SMAFA_ERR_PANIC ? 101 : 1;
    }
    // Everything has been written (rows go out through write(2)) and every handle is closed: leave without running
    // the HIP runtime's exit handlers, which cost a noticeable part of a sub-second run.
    fflush(stdout);
    fflush(stderr);
    if (getenv("SMAFA_NO_FAST_EXIT")) return code;  // under a profiler: its tool library writes its files from an exit handler
    _exit(code);
}
