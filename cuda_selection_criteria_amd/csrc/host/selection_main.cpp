// selection_main.cpp -- `selection`: drop-in for the reference's GPU selection driver
// (src/selection_cuda.cpp:59-189; README.md:60-66 documents it as `selection -l -h -a -b`),
// producing the OUTPUT of the reference's CPU program src/selection.cpp:228-300 (criterion smh_a):
// lines "fn1 fn2 <jaccard %f>" in rank order.
//
//   -l <file>   list of genome paths; <path>.hll and <path>.smh<m> must exist (written by build_sketch)
//   -h <tau>    similarity threshold (float, std::stof like selection.cpp:103)
//   -a <bytes>  auxiliary memory per genome; m = bytes/8 SuperMinHash buckets (selection.cpp:231)
//   -b <n>      accepted for CLI compatibility (CUDA block size in the reference); ignored
//   -c <crit>   smh_a (default; the only criterion of the reference's GPU driver, selection_cuda.cpp:64), or hll_a /
//               hll_an as in the CPU program (src/selection.cpp:122-227: auxiliary HLL p = ctz(aux_bytes), file .hll_<p>), or
//               none: no criterion in front of the Jaccard test -- every pair inside the CB bound (with -n: every pair); reads
//               only the .hll files, -a is not needed (SELHIP_CRIT_NONE: the reference README's "CB criterion" / "no criterion" lines)
//               smh_c: at least -C <c_min> of the m = -a bytes / 8 SuperMinHash buckets equal (SELHIP_CRIT_SMH_C: the SuperMinHash
//               estimate c / m >= c_min / m, exhaustive, no banding); -a and -C (or -G) must be given; with -l, -q, -p, -k, -K, -n, not with -g or -B
//   -C <c_min>  the count threshold of -c smh_c (1 .. m), an option of that criterion alone
//   -G <gamma>  the minimum containment of -c smh_c, an option of that criterion alone, in -C's place or beside it: a pair passes with
//               at least ceil(gamma m a / (a + b - gamma a)) equal buckets, a <= b its two cardinalities -- the count at which the
//               SuperMinHash estimate of the smaller genome's containment is gamma (selhip_ctx_set_min_containment) -- and, with -C,
//               at least c_min.  The prefilter of -n -S max_containment -h gamma; with -l, -q, -p, -k, -K
//   -t <n>      host threads for loading sketches (selection.cpp:97)
//   -g <n>      number of GPUs to shard the pair space over (default 1; any criterion); selected pairs gathered over RCCL/xGMI
//   -n          no CB pruning ("smh_a" mode of experiments/src/time_smh.cpp:229-257)
//   -A <algo>   stage-1 algorithm: auto | stream | sig | hashjoin (sort-based: same result, sub-quadratic); with -q also
//               index (the database's band signatures sorted once, one search per query and band; band shapes of sig)
//   -F <0|1>    estimator flavour: 1 = FMA (reference Makefile build on FMA hosts, default), 0 = strict
//   -B <n>      out-of-core: keep the sketches in host memory and process the pair space in blocks of n genomes
//               (selhip_ooc_select; same output); 0 = everything resident on the device (default)
//   -o <file>   write the result as a binary result file (include/selection_host.h: "SELR" format: records + name table)
//               instead of text on stdout
//   -r <file>   no selection: print the text form of a result file written with -o (needs no GPU)
//   -q <file>   query-vs-database selection: -q lists the query genomes, -l the database; prints "query_path db_path J" per
//               selected pair (one member in each list) in (query rank, database rank) order (selhip_ctx_run_queries; criterion
//               smh_a, hll_a, hll_an or none -- for hll_a / hll_an the .hll_<p> files of both lists are read; one device -- not combinable
//               with -g, -B, -o or -r)
//   -k <n>      with -q: only every query's n best pairs (1..1024), cut on the device (selhip_ctx_set_query_topk), printed in ranked
//               order: query rank, then J descending, ties by database rank.  The best among the pairs that pass -c and -h, not an
//               unconditional nearest-neighbour search (for that: -c none -n and a -h below every J, e.g. -1)
//   -K <n>      all-pairs selection (-l alone): only every genome's n best partners (1..1024), cut on the device
//               (selhip_ctx_set_allpairs_topk), printed as "owner_path partner_path J" in ranked order: owner rank, then J descending, ties
//               by partner rank.  A selected pair counts for both of its genomes, so it can be printed twice, once or not at all.  The
//               best among the pairs that pass -c and -h (every genome's exact nearest neighbours: -c none -n -h -1); one device, text
//               output -- not combinable with -q (per-query cut: -k), -g, -B, -o or -r
//   -R <rows>   with -K -c smh_c -V smh: the pass runs in rounds of that many rows (or `auto`: the largest R with R n <= 2^27), each merged
//               into a carried list of at most n best partners per genome whose n-th values prune the next round at the source
//               (selhip_ctx_set_topk_rounds): the same text, with memory for n K records and one round instead of every pair that
//               shares a bucket, and no limit of 2^30 such pairs.  Not combinable with -q, -p, -M, -g or -B; needs -K
//   -p <file>   pair-list selection: only the pairs listed in the file, lines "path1 path2[ anything]" with paths of the -l list in
//               either order -- the lines this program prints, so one run's output is the next run's pair file
//               (selhip_ctx_run_pairs: a pair listed twice is printed twice).  With every -c, -n, -F, -o and -A auto|sig|stream; one
//               device -- not combinable with -q, -k, -K, -B or -g above 1
//   -M <file>   no selection pass: the dense similarity matrix of the -l list (with -q: rows = the -q list, columns = the -l list) as a
//               tab-separated table in FILE-LIST order (selhip_ctx_matrix / selhip_ctx_query_matrix, selhost_write_matrix): first line a
//               tab and the column names, then per row its name and the values in %.17g.  Jaccard estimates (1 on the diagonal, nan for
//               two empty sketches); with -U the union sizes.  Reads only the .hll files (-a and -b are accepted and unused); with -F and
//               -t -- not combinable with -p, -k, -K, -g, -B, -o, -r, nor with the options of a selection pass -h, -c, -n, -A
//   -U          with -M: the union estimate U of every pair instead of J
//   -E <est>    with -M: the estimator behind the cells.  hll (default): the HyperLogLog values above.  smh: the SuperMinHash estimate of
//               J, (equal buckets of the pair) / m; smh_matches: that count itself, printed as an integer (SELHIP_MEASURE_SMH_JACCARD /
//               _SMH_MATCHES).  smh and smh_matches read the .smh<m> files too, m = -a bytes / 8: -a must be given, -U is refused
//   -S <name>   the measure.  Of a selection pass (-l, -q, -p, -k, -K; -c smh_a | none | smh_c): jaccard (default) or max_containment --
//               the pairs whose intersection estimate I = e_1 + e_2 - U is at least -h of the SMALLER genome, I / min(e_1, e_2),
//               printed in J's place (selhip_ctx_set_measure): a plasmid, phage or fragment inside a genome.  max_containment needs -n
//               (the CB bound is a bound on J) and takes no -c hll_a | hll_an (bounds on J), no -g, -B (the drivers carry no measure)
//               and no -o (the result file records no measure).  With -M: intersection (I), containment (I / e_row: the share of the
//               row genome found in the column genome, with -q the query inside the database genome) or max_containment (jaccard: the
//               default table); a value of -E hll -- not with -U or -E smh | smh_matches
//   -V <est>    the estimator behind the value that a selection pass under -c smh_c tests against -h and prints (selhip_ctx_set_estimator).
//               hll (default): the HyperLogLog value, as ever.  smh: the SuperMinHash estimate of the count c the criterion computes
//               anyway -- c / m, under -S max_containment c (a + b) / ((m + c) a), a <= b the pair's cardinalities -- with no HLL stage
//               behind the count: a pair is printed when c passes -C / -G AND that value is at least -h.  The sparse list of pairs by
//               SuperMinHash J, and with -K / -k the nearest neighbours by it (-c smh_c -C 1 -n -h -1 -K 10 -V smh).  With -l, -q, -p,
//               -k, -K, -n, -S max_containment, -o; -V smh needs -c smh_c and takes no -M (its estimator is -E), -g or -B
//   -D          with -c hll_a | hll_an: derive the auxiliary HLL sketches instead of reading them -- no .hll_<p> file is opened; the p =
//               ctz(-a bytes) sketches are folded on the device from the .hll registers (selhip_ctx_fold_aux_hll: bit for bit the
//               registers of the files, so the same output), for any p in 4..14.  With -l, -q (both lists), -p, -k, -K; with -g and
//               -B the host twin (selhost_hll_fold) folds the array handed to the drivers.  Not with -c smh_a | smh_c | none (they
//               read no auxiliary HLL sketch), -M or -r
//   -L <file>   behind the selection pass: its single-linkage clusters, computed on the device from the result list (selhip_ctx_cluster)
//               and written to <file>, one line per genome of the -l list in file-list order:
//               path <TAB> cluster <TAB> cluster_size <TAB> degree <TAB> representative_path   (cluster: dense id by ascending smallest
//               rank; degree: records the genome appears in).  Stdout stays byte for byte what it is without -L.  With -l under every
//               -c, with -p, and with -K (with or without -R: the k-NN graph, directed records as undirected edges); one device -- not
//               combinable with -q (two index spaces), -M, -g, -B (their lists live on the host) or -r
//   -T <value>  with -L: only the selected pairs whose printed value is at least this (f64) are edges -- one pass at a low -h can be
//               clustered at several levels; default: every selected pair
//   -Y <rule>   with -L: the representative of a cluster: max_degree (default; most records, ties to the smaller rank), min_rank (the
//               smallest genome) or max_rank (the largest)
//   -Z <how>    with -L: single (default: the single-linkage clusters above) or greedy: the greedy representative clusters of the selected
//               pairs (selhip_ctx_cluster_greedy; CD-HIT / UCLUST): the genomes are visited in the order -Y names (max_degree, default: the
//               most records first; min_rank; max_rank: the largest sketch first) and one becomes a representative unless a selected pair
//               (with -T: of at least that value) already joins it to one; every other genome goes to the representative it has the
//               greatest value with.  The table gains a sixth column:
//               path <TAB> cluster <TAB> cluster_size <TAB> degree <TAB> representative_path <TAB> value_to_representative
//               (cluster: dense id by ascending representative rank; the value printed as std::to_string does, 1.000000 for a representative)
//   -W <file>   with -L -Z greedy: the visiting order is a score per genome, the greatest first (ties to the smaller genome): lines of
//               path <TAB> unsigned score (up to 2^32 - 1), one per genome of the -l list, in any order; read and checked before any
//               device work.  Not with -Y
//   -P <dir>    one merged sketch set per group, written into <dir> (created if missing): the union sketch of the group's genomes, merged on
//               the device (selhip_ctx_merge_groups: the maximum of the HLL registers, the minimum of the SuperMinHash buckets -- bit for
//               bit the sketches build_sketch would write for the members' records in one FASTA).  <dir>/<name>.hll, <dir>/<name>.smh<m>
//               where the run reads .smh<m> files (-c smh_a | smh_c), <dir>/<name>.hll_<p> where it reads or folds auxiliary sketches
//               (-c hll_a | hll_an), and <dir>/filelist.txt, one <dir>/<name> per line in group order: the directory is a database for
//               selection -l <dir>/filelist.txt [-q ...].  The groups come from -L or from -I:
//               with -L: the clusters of that run (-Z, -T, -Y, -W as ever); <name> is cluster_<id>, zero-padded to the width of the largest
//               id.  Stdout and the -L table stay byte for byte what they are without -P.
//               Not without -L or -I, and not with -q, -M, -g, -B or -r
//   -I <file>   with -P and without -L: the groups are read from <file>, no pass runs (as with -M): lines path <TAB> group_name, the
//               groups numbered by first appearance, <name> = group_name (not empty, no '/'); a path that is not in the -l list is a
//               format error with its line number; a genome of the list that the file does not name is in no group.  -c and -a say which
//               sketch files are in play, as for a pass.  Not with -L, -p, -k, -K or -o
//   -N <file>   no selection pass (as with -M): the agglomerative hierarchy of the genomes of the -l list, computed on the device from the
//               dense matrix under the distance 1 - similarity (selhip_ctx_linkage), written to <file> as an ultrametric Newick tree
//               with the list's paths as leaf names: a node stands at its merge's height, a branch has the length (parent's height -
//               own height) / 2.  The similarity is that of -M: Jaccard by default, -E smh -a bytes (SuperMinHash), -S max_containment;
//               not -U, -E smh_matches, -S intersection | containment (no symmetric similarity).  May stand beside -M (both are
//               written); not with -q, -p, -g, -B, -r, -k, -K, -o, -L, -H, -P, -D or an option of a selection pass
//   -J <file>   the merges of the same hierarchy, one line each in the order the device emitted them (children before parents):
//               path_a <TAB> path_b <TAB> height <TAB> size   (the merged cluster lives on under path_a, its smallest rank; the height
//               printed as std::to_string does).  Alone or beside -N
//   -X <method> with -N / -J: average (default, UPGMA), complete, weighted (WPGMA) or single
//   -x          usage
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../../include/selection_hip.h"
#include "../../../include/selection_host.h"

// -c smh_c: its thresholds onto the context -- -C c_min (0: not given) and -G gamma (NaN: not given)
// and its estimator (-V)
static double g_min_containment = std::nan("");
static int g_estimator = SELHIP_ESTIMATOR_HLL;
static bool g_fold_aux = false;                  // -D: the auxiliary HLL sketches are folded from the main ones, no .hll_<p> file is read
static long long g_topk_rounds = 0;              // -R: rows per round of -K (0: not given, SELHIP_TOPK_ROUNDS_AUTO: auto)
static std::string g_cluster_file = "";         // -L: the cluster table of the pass's result list goes here ("" = none)
static double g_cluster_min = -INFINITY;         // -T: records below this value are no edges
static int g_cluster_rep = SELHIP_REP_MAX_DEGREE;   // -Y
static bool g_cluster_greedy = false;            // -Z greedy
static std::string g_priority_file = "";        // -W: the scores that order the greedy clusters ("" = none)
static std::vector<uint32_t> g_priority;         // ... in rank order, read by load_priorities
static std::string g_merge_dir = "";            // -P: one merged sketch set per group goes into this directory ("" = none)
static std::string g_groups_file = "";          // -I: the groups of -P, read from this file ("" = the clusters of -L)
static std::string g_forest_file = "";         // -H: the maximum spanning forest of the pass's result list goes here ("" = none)
static std::string g_newick_file = "", g_merges_file = "";   // -N, -J: the hierarchy of the dense matrix as a tree / as its merges ("" = none)
static unsigned g_merge_m = 0, g_merge_p_aux = 0;   // the SuperMinHash buckets and the auxiliary precision in play in the run (0 = none)

// -P: the sketches of the context's set merged by d_group (device, rank order) into n_groups sets named names[], written into g_merge_dir
static int write_merged(selhip_ctx* ctx, const int32_t* d_group, int64_t n_groups, const std::vector<std::string>& names) {
    const size_t G = (size_t)n_groups, hb = (size_t)1 << 14, ab = g_merge_p_aux ? (size_t)1 << g_merge_p_aux : 0, m = g_merge_m;
    std::vector<uint8_t> hll(G * hb), aux_hll(G * ab);
    std::vector<uint64_t> smh(G * m);
    selhip_merged_t out{nullptr, nullptr, nullptr, nullptr, nullptr};
    void* d = nullptr;
    int r = G ? selhip_malloc(&d, G * (hb + ab + m * 8)) : 0;
    if (!r && G) {
        // the byte rows first: both stay 16-byte aligned, the buckets behind them 8-byte aligned
        out.d_hll = static_cast<uint8_t*>(d);
        if (ab) out.d_aux_hll = out.d_hll + G * hb;
        if (m) out.d_aux = reinterpret_cast<uint64_t*>(out.d_hll + G * (hb + ab));
    }
    if (!r) r = selhip_ctx_merge_groups(ctx, d_group, n_groups, &out);
    if (!r && G) r = selhip_memcpy_d2h(hll.data(), out.d_hll, G * hb);
    if (!r && G && ab) r = selhip_memcpy_d2h(aux_hll.data(), out.d_aux_hll, G * ab);
    if (!r && G && m) r = selhip_memcpy_d2h(smh.data(), out.d_aux, G * m * 8);
    if (d) selhip_free(d);
    if (r) return r;
    mkdir(g_merge_dir.c_str(), 0777);                                           // (exists already: fine; anything else shows at the first file)
    std::string list;
    int hr = 0;
    for (size_t c = 0; c < G && !hr; ++c) {
        const std::string base = g_merge_dir + "/" + names[c];
        hr = selhost_write_hll((base + ".hll").c_str(), hll.data() + c * hb, 14);
        if (!hr && m) hr = selhost_write_smh((base + ".smh" + std::to_string(m)).c_str(), smh.data() + c * m, (uint32_t)m);
        if (!hr && ab) hr = selhost_write_hll((base + ".hll_" + std::to_string(g_merge_p_aux)).c_str(), aux_hll.data() + c * ab, g_merge_p_aux);
        list += base + "\n";
    }
    if (hr) { std::cerr << "selection: -P: " << selhost_last_error() << "\n"; return 5; }
    std::ofstream f(g_merge_dir + "/filelist.txt", std::ios::binary);
    f << list;
    f.close();
    if (!f) { std::cerr << "selection: -P: cannot write '" << g_merge_dir << "/filelist.txt'\n"; return 5; }
    return 0;
}

// -L ... -P: the clusters as groups, named cluster_<id> zero-padded to the width of the largest id
static int write_merged_clusters(selhip_ctx* ctx, const int32_t* d_cluster, int64_t n_clusters) {
    if (g_merge_dir.empty()) return 0;
    const size_t width = std::to_string(n_clusters > 0 ? n_clusters - 1 : 0).size();
    std::vector<std::string> names((size_t)n_clusters);
    for (int64_t c = 0; c < n_clusters; ++c) {
        const std::string id = std::to_string(c);
        names[(size_t)c] = "cluster_" + std::string(width - id.size(), '0') + id;
    }
    return write_merged(ctx, d_cluster, n_clusters, names);
}

// -W: the scores of the n genomes of ds, checked on the host; 0 = fine (or no -W)
static int load_priorities(const selhost_dataset* ds, int64_t n) {
    if (g_priority_file.empty()) return 0;
    std::ifstream f(g_priority_file, std::ios::binary);
    if (!f) { std::cerr << "selection: -W: cannot read '" << g_priority_file << "'\n"; return 5; }
    std::unordered_map<std::string, int64_t> rank_of;
    for (int64_t g = 0; g < n; ++g) rank_of.emplace(selhost_dataset_name(ds, g), g);
    g_priority.assign((size_t)n, 0);
    std::vector<char> seen((size_t)n, 0);
    int64_t n_seen = 0, line_no = 0;
    std::string line;
    while (std::getline(f, line)) {
        ++line_no;
        if (line.empty()) continue;
        const size_t tab = line.find('\t');
        const std::string score = tab == std::string::npos ? "" : line.substr(tab + 1);
        const auto it = tab == std::string::npos ? rank_of.end() : rank_of.find(line.substr(0, tab));
        const bool digits = !score.empty() && score.size() <= 10 && score.find_first_not_of("0123456789") == std::string::npos;
        const unsigned long long v = digits ? std::strtoull(score.c_str(), nullptr, 10) : 0;
        if (it == rank_of.end() || !digits || v > 0xFFFFFFFFull || seen[(size_t)it->second]) {
            std::cerr << "selection: -W: line " << line_no << " of '" << g_priority_file
                      << "' is not 'path<TAB>unsigned score' for a genome of the -l list not scored yet\n";
            return 5;
        }
        seen[(size_t)it->second] = 1;
        g_priority[(size_t)it->second] = (uint32_t)v;
        ++n_seen;
    }
    if (n_seen != n) { std::cerr << "selection: -W: '" << g_priority_file << "' scores " << n_seen << " of the " << n << " genomes of the -l list\n"; return 5; }
    return 0;
}

// -L -Z greedy: the greedy representative clusters of the result list as a table in file-list order
static int write_greedy(selhip_ctx* ctx, const selhost_dataset* ds, int64_t n) {
    std::vector<int32_t> rep_of((size_t)n), cluster((size_t)n), degree((size_t)n), size((size_t)n);
    std::vector<double> value((size_t)n);
    selhip_greedy_t out{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    void* d = nullptr;
    int64_t n_clusters = 0;
    const bool scored = !g_priority_file.empty();
    // value[n] (f64) first, then rep_of, cluster, degree, cluster_size and the scores: 4-byte words
    int r = n ? selhip_malloc(&d, (size_t)n * (sizeof(double) + 5 * sizeof(int32_t))) : 0;
    uint32_t* d_priority = nullptr;
    if (!r && n) {
        out.d_value = static_cast<double*>(d);
        int32_t* base = reinterpret_cast<int32_t*>(out.d_value + n);
        out.d_rep_of = base; out.d_cluster = base + n; out.d_degree = base + 2 * n; out.d_cluster_size = base + 3 * n;
        d_priority = reinterpret_cast<uint32_t*>(base + 4 * n);
        if (scored) r = selhip_memcpy_h2d(d_priority, g_priority.data(), (size_t)n * sizeof(uint32_t));
    }
    // (without a genome there is no array to point to: the rule the call accepts with a NULL d_priority)
    if (!r) r = selhip_ctx_cluster_greedy(ctx, g_cluster_min, scored && n ? SELHIP_REP_PRIORITY : g_cluster_rep, scored && n ? d_priority : nullptr, &out, &n_clusters);
    if (!r && n) r = selhip_memcpy_d2h(value.data(), out.d_value, (size_t)n * sizeof(double));
    if (!r && n) r = selhip_memcpy_d2h(rep_of.data(), out.d_rep_of, (size_t)n * sizeof(int32_t));
    if (!r && n) r = selhip_memcpy_d2h(cluster.data(), out.d_cluster, (size_t)n * sizeof(int32_t));
    if (!r && n) r = selhip_memcpy_d2h(degree.data(), out.d_degree, (size_t)n * sizeof(int32_t));
    if (!r && n_clusters) r = selhip_memcpy_d2h(size.data(), out.d_cluster_size, (size_t)n_clusters * sizeof(int32_t));
    if (!r) r = write_merged_clusters(ctx, out.d_cluster, n_clusters);
    if (d) selhip_free(d);
    if (r) return r;
    std::vector<int64_t> rank_of_line((size_t)n);
    for (int64_t g = 0; g < n; ++g) rank_of_line[(size_t)selhost_dataset_order(ds, g)] = g;
    std::ofstream f(g_cluster_file, std::ios::binary);
    for (int64_t line = 0; line < n; ++line) {
        const int64_t g = rank_of_line[(size_t)line];
        const int32_t c = cluster[(size_t)g];
        f << selhost_dataset_name(ds, g) << '\t' << c << '\t' << size[(size_t)c] << '\t' << degree[(size_t)g] << '\t'
          << selhost_dataset_name(ds, rep_of[(size_t)g]) << '\t' << std::to_string(value[(size_t)g]) << '\n';
    }
    f.close();
    if (!f) { std::cerr << "selection: -L: cannot write '" << g_cluster_file << "'\n"; return 5; }
    return 0;
}

// -H: behind a finished pass of ctx over the n genomes of ds, the maximum spanning forest of its result list (the single-linkage
// dendrogram's merges), one line per edge, best first: path_a<TAB>path_b<TAB>value
static int write_forest(selhip_ctx* ctx, const selhost_dataset* ds, int64_t n) {
    if (g_forest_file.empty()) return 0;
    const size_t cap = n > 1 ? (size_t)(n - 1) : 0;
    std::vector<selhip_pair_t> edges(cap);
    selhip_forest_t out{nullptr, nullptr};
    void* d = nullptr;
    int64_t n_edges = 0;
    int r = cap ? selhip_malloc(&d, cap * sizeof(selhip_pair_t)) : 0;
    if (!r) out.d_edges = static_cast<selhip_pair_t*>(d);
    if (!r) r = selhip_ctx_spanning_forest(ctx, g_cluster_min, &out, &n_edges);
    if (!r && n_edges) r = selhip_memcpy_d2h(edges.data(), out.d_edges, (size_t)n_edges * sizeof(selhip_pair_t));
    if (d) selhip_free(d);
    if (r) return r;
    std::ofstream f(g_forest_file, std::ios::binary);
    for (int64_t e = 0; e < n_edges; ++e)
        f << selhost_dataset_name(ds, edges[(size_t)e].i) << '\t' << selhost_dataset_name(ds, edges[(size_t)e].k) << '\t'
          << std::to_string(edges[(size_t)e].jaccard) << '\n';
    f.close();
    if (!f) { std::cerr << "selection: -H: cannot write '" << g_forest_file << "'\n"; return 5; }
    return 0;
}

// -L (and -H, first): behind a finished pass of ctx over the n genomes of ds, the clusters of its result list as a table in file-list order
static int write_clusters(selhip_ctx* ctx, const selhost_dataset* ds, int64_t n) {
    if (const int r = write_forest(ctx, ds, n)) return r;
    if (g_cluster_file.empty()) return 0;
    if (g_cluster_greedy) return write_greedy(ctx, ds, n);
    std::vector<int32_t> cluster((size_t)n), degree((size_t)n), size((size_t)n), rep((size_t)n);
    selhip_clusters_t out{nullptr, nullptr, nullptr, nullptr, nullptr};
    void* d = nullptr;
    int64_t n_clusters = 0;
    int r = n ? selhip_malloc(&d, (size_t)n * 4 * sizeof(int32_t)) : 0;
    if (!r && n) {
        int32_t* base = static_cast<int32_t*>(d);
        out.d_cluster = base; out.d_degree = base + n; out.d_cluster_size = base + 2 * n; out.d_cluster_rep = base + 3 * n;
    }
    if (!r) r = selhip_ctx_cluster(ctx, g_cluster_min, g_cluster_rep, &out, &n_clusters);
    if (!r && n) r = selhip_memcpy_d2h(cluster.data(), out.d_cluster, (size_t)n * sizeof(int32_t));
    if (!r && n) r = selhip_memcpy_d2h(degree.data(), out.d_degree, (size_t)n * sizeof(int32_t));
    if (!r && n_clusters) r = selhip_memcpy_d2h(size.data(), out.d_cluster_size, (size_t)n_clusters * sizeof(int32_t));
    if (!r && n_clusters) r = selhip_memcpy_d2h(rep.data(), out.d_cluster_rep, (size_t)n_clusters * sizeof(int32_t));
    if (!r) r = write_merged_clusters(ctx, out.d_cluster, n_clusters);
    if (d) selhip_free(d);
    if (r) return r;
    std::vector<int64_t> rank_of_line((size_t)n);
    for (int64_t g = 0; g < n; ++g) rank_of_line[(size_t)selhost_dataset_order(ds, g)] = g;
    std::ofstream f(g_cluster_file, std::ios::binary);
    for (int64_t line = 0; line < n; ++line) {
        const int64_t g = rank_of_line[(size_t)line];
        const int32_t c = cluster[(size_t)g];
        f << selhost_dataset_name(ds, g) << '\t' << c << '\t' << size[(size_t)c] << '\t' << degree[(size_t)g] << '\t'
          << selhost_dataset_name(ds, rep[(size_t)c]) << '\n';
    }
    f.close();
    if (!f) { std::cerr << "selection: -L: cannot write '" << g_cluster_file << "'\n"; return 5; }
    return 0;
}

static int set_count_thresholds(selhip_ctx* ctx, int min_matches) {
    int r = min_matches > 0 ? selhip_ctx_set_min_matches(ctx, min_matches) : 0;
    if (!r && !std::isnan(g_min_containment)) r = selhip_ctx_set_min_containment(ctx, g_min_containment);
    if (!r) r = selhip_ctx_set_estimator(ctx, g_estimator);
    return r;
}

// the auxiliary HLL sketches of the context's database (queries: of its query set): folded on the device under -D, else uploaded
static int load_aux_hll(selhip_ctx* ctx, const selhost_dataset* ds, unsigned p_aux, bool queries) {
    if (g_fold_aux) return queries ? selhip_ctx_fold_queries_aux_hll(ctx, (int)p_aux) : selhip_ctx_fold_aux_hll(ctx, (int)p_aux);
    return queries ? selhip_ctx_upload_queries_aux_hll(ctx, selhost_dataset_aux_hll(ds), (int)p_aux)
                   : selhip_ctx_upload_aux_hll(ctx, selhost_dataset_aux_hll(ds), (int)p_aux);
}
// precision of the .hll_<p> files a run opens: none under -D
static unsigned aux_files(unsigned p_aux) { return g_fold_aux ? 0 : p_aux; }

// -q: the query list against the database list (-l), both loaded and sorted by cardinality; text on stdout.  criterion: "smh_a"
// (m = aux_bytes / 8 buckets), "hll_a" / "hll_an" (auxiliary HLL p = ctz(aux_bytes), as the all-pairs mode) or "none" (.hll files only)
static int run_queries(const std::string& query_file, const std::string& db_file, const std::string& criterion, float threshold,
                       int aux_bytes, int mode, int algo, int fp_mode, int threads, int top_k, int min_matches, int measure) {
    const bool smh = criterion == "smh_a";
    const bool smh_c = criterion == "smh_c";
    const bool none = criterion == "none";
    const int crit = smh ? SELHIP_CRIT_SMH_A : smh_c ? SELHIP_CRIT_SMH_C : none ? SELHIP_CRIT_NONE : criterion == "hll_a" ? SELHIP_CRIT_HLL_A : SELHIP_CRIT_HLL_AN;
    const unsigned m = smh || smh_c ? (unsigned)aux_bytes / 8 : 0;
    const unsigned p_aux = smh || smh_c || none ? 0 : (unsigned)__builtin_ctz(aux_bytes ? aux_bytes : 1);
    // (smh_a keeps the messages it always had; an hll criterion names the mode and the criterion)
    const std::string what = smh ? "" : "selection: -q -c " + criterion + ": ";
    selhost_dataset* db = nullptr;
    selhost_dataset* qs = nullptr;
    if (selhost_dataset_load(&db, db_file.c_str(), m, aux_files(p_aux), fp_mode, threads)) {
        if (!smh) std::cerr << what << "cannot read database list '" << db_file << "': ";
        std::cerr << selhost_last_error() << "\n";
        return 1;
    }
    if (selhost_dataset_load(&qs, query_file.c_str(), m, aux_files(p_aux), fp_mode, threads)) {
        if (!smh) std::cerr << what << "cannot read query list '" << query_file << "': ";
        std::cerr << selhost_last_error() << "\n";
        selhost_dataset_free(db);
        return 1;
    }
    int n_rows = 1, n_bands = 1;
    if (m) selhost_banding(m, threshold, SELHOST_BANDING_CPU, &n_rows, &n_bands);
    // hll_a / hll_an do not read SuperMinHash buckets: a one-bucket placeholder keeps the upload calls uniform
    const int64_t n_db = selhost_dataset_size(db), n_qs = selhost_dataset_size(qs);
    std::vector<uint64_t> no_smh(m ? 0 : (size_t)std::max<int64_t>(1, std::max(n_db, n_qs)), 0);
    std::vector<selhip_pair_t> pairs;
    selhip_ctx* ctx = nullptr;
    int r = selhip_device_count() > 0 ? selhip_ctx_create(&ctx, 0) : SELHIP_E_NODEVICE;
    if (r) {
        std::cerr << (smh ? "selection: " : what) << "no MI355X (gfx950) device available: " << selhip_last_error(nullptr) << "\n";
        selhost_dataset_free(db); selhost_dataset_free(qs);
        return 3;
    }
    selhip_ctx_set_fp_mode(ctx, fp_mode);
    r = selhip_ctx_upload(ctx, selhost_dataset_hll(db), m ? selhost_dataset_aux(db) : no_smh.data(), selhost_dataset_cards(db), n_db,
                          m ? (int)m : 1, 14);
    if (!r) r = selhip_ctx_upload_queries(ctx, selhost_dataset_hll(qs), m ? selhost_dataset_aux(qs) : no_smh.data(), selhost_dataset_cards(qs), n_qs);
    if (!r && p_aux) r = load_aux_hll(ctx, db, p_aux, false);
    if (!r && p_aux) r = load_aux_hll(ctx, qs, p_aux, true);
    if (!r) r = selhip_ctx_set_criterion(ctx, crit);
    if (!r && smh_c) r = set_count_thresholds(ctx, min_matches);
    if (!r) r = selhip_ctx_set_measure(ctx, measure);
    if (!r && top_k) r = selhip_ctx_set_query_topk(ctx, top_k);
    if (!r) r = selhip_ctx_run_queries(ctx, mode, algo, threshold, n_rows, n_bands);
    if (!r) {
        pairs.resize((size_t)selhip_ctx_result_count(ctx));
        r = top_k ? selhip_ctx_fetch_ranked(ctx, pairs.data(), (int64_t)pairs.size()) : selhip_ctx_fetch(ctx, pairs.data(), (int64_t)pairs.size());
    }
    if (r) std::cerr << (smh ? "selection: " : what) << selhip_last_error(ctx) << "\n";
    selhip_ctx_destroy(ctx);
    if (!r) {
        std::string out;
        char line[8192];
        for (const selhip_pair_t& pr : pairs) {
            const int w = selhost_format_line(selhost_dataset_name(qs, pr.i), selhost_dataset_name(db, pr.k), pr.jaccard, line, sizeof line);
            if (w > 0) out.append(line, (size_t)w);
        }
        std::cout << out;
    }
    selhost_dataset_free(db);
    selhost_dataset_free(qs);
    return r ? 4 : 0;
}

// -K: one all-pairs pass over the list with the device-side cut on; text on stdout, one line per kept (owner, partner) record
static int run_neighbours(const std::string& list_file, int crit, float threshold, int aux_bytes, int mode, int algo, int fp_mode,
                          int threads, int top_k, int min_matches, int measure) {
    const bool reads_smh = crit == SELHIP_CRIT_SMH_A || crit == SELHIP_CRIT_SMH_C;
    const unsigned m = reads_smh ? (unsigned)aux_bytes / 8 : 0;
    const unsigned p_aux = reads_smh || crit == SELHIP_CRIT_NONE ? 0 : (unsigned)__builtin_ctz(aux_bytes ? aux_bytes : 1);
    g_merge_m = m; g_merge_p_aux = p_aux;
    selhost_dataset* ds = nullptr;
    if (selhost_dataset_load(&ds, list_file.c_str(), m, aux_files(p_aux), fp_mode, threads)) { std::cerr << selhost_last_error() << "\n"; return 1; }
    const int64_t n = selhost_dataset_size(ds);
    if (const int w = load_priorities(ds, n)) { selhost_dataset_free(ds); return w; }
    int n_rows = 1, n_bands = 1;
    if (m) selhost_banding(m, threshold, SELHOST_BANDING_CPU, &n_rows, &n_bands);
    std::vector<uint64_t> no_smh(m ? 0 : (size_t)(n > 0 ? n : 1), 0);
    std::vector<selhip_pair_t> pairs;
    selhip_ctx* ctx = nullptr;
    int r = selhip_device_count() > 0 ? selhip_ctx_create(&ctx, 0) : SELHIP_E_NODEVICE;
    if (r) {
        std::cerr << "selection: no MI355X (gfx950) device available: " << selhip_last_error(nullptr) << "\n";
        selhost_dataset_free(ds);
        return 3;
    }
    selhip_ctx_set_fp_mode(ctx, fp_mode);
    r = selhip_ctx_upload(ctx, selhost_dataset_hll(ds), m ? selhost_dataset_aux(ds) : no_smh.data(), selhost_dataset_cards(ds), n, m ? (int)m : 1, 14);
    if (!r && p_aux) r = load_aux_hll(ctx, ds, p_aux, false);
    if (!r) r = selhip_ctx_set_criterion(ctx, crit);
    if (!r && crit == SELHIP_CRIT_SMH_C) r = set_count_thresholds(ctx, min_matches);
    if (!r) r = selhip_ctx_set_measure(ctx, measure);
    if (!r) r = selhip_ctx_set_allpairs_topk(ctx, top_k);
    if (!r && g_topk_rounds) r = selhip_ctx_set_topk_rounds(ctx, g_topk_rounds);
    if (!r) r = selhip_ctx_run(ctx, mode, algo, threshold, n_rows, n_bands, 0, n);
    if (!r) {
        pairs.resize((size_t)selhip_ctx_result_count(ctx));
        r = selhip_ctx_fetch_ranked(ctx, pairs.data(), (int64_t)pairs.size());
    }
    if (!r) r = write_clusters(ctx, ds, n);
    if (r) std::cerr << "selection: " << selhip_last_error(ctx) << "\n";
    selhip_ctx_destroy(ctx);
    if (!r) {
        std::string out;
        char line[8192];
        for (const selhip_pair_t& pr : pairs) {
            const int w = selhost_format_line(selhost_dataset_name(ds, pr.i), selhost_dataset_name(ds, pr.k), pr.jaccard, line, sizeof line);
            if (w > 0) out.append(line, (size_t)w);
        }
        std::cout << out;
    }
    selhost_dataset_free(ds);
    return r ? 4 : 0;
}

// -M: the dense matrix of one list, or of the query list against the database list, written as text in file-list order
// measure: a SELHIP_MEASURE_* code; m: the SuperMinHash buckets to load for the SMH measures, 0 for the HLL ones (only the .hll files)
static int run_matrix(const std::string& list_file, const std::string& query_file, const std::string& out_file, int measure, unsigned m,
                      int fp_mode, int threads) {
    selhost_dataset* db = nullptr;
    selhost_dataset* qs = nullptr;
    if (selhost_dataset_load(&db, list_file.c_str(), m, 0, fp_mode, threads)) { std::cerr << "selection: -M: " << selhost_last_error() << "\n"; return 1; }
    if (!query_file.empty() && selhost_dataset_load(&qs, query_file.c_str(), m, 0, fp_mode, threads)) {
        std::cerr << "selection: -M: cannot read query list '" << query_file << "': " << selhost_last_error() << "\n";
        selhost_dataset_free(db);
        return 1;
    }
    const selhost_dataset* rows = qs ? qs : db;
    const int64_t n_d = selhost_dataset_size(db), n_r = selhost_dataset_size(rows);
    // the positions: rank -> line of the file list; the names in file order
    std::vector<int32_t> col_pos((size_t)n_d), row_pos((size_t)n_r);
    std::vector<const char*> col_names((size_t)n_d), row_names((size_t)n_r);
    for (int64_t r = 0; r < n_d; ++r) { col_pos[(size_t)r] = (int32_t)selhost_dataset_order(db, r); col_names[(size_t)col_pos[(size_t)r]] = selhost_dataset_name(db, r); }
    for (int64_t r = 0; r < n_r; ++r) { row_pos[(size_t)r] = (int32_t)selhost_dataset_order(rows, r); row_names[(size_t)row_pos[(size_t)r]] = selhost_dataset_name(rows, r); }
    std::vector<double> values((size_t)n_r * (size_t)n_d);
    std::vector<uint64_t> no_smh(m ? 0 : (size_t)std::max<int64_t>(1, std::max(n_d, n_r)), 0);
    selhip_ctx* ctx = nullptr;
    int r = selhip_device_count() > 0 ? selhip_ctx_create(&ctx, 0) : SELHIP_E_NODEVICE;
    if (r) {
        std::cerr << "selection: no MI355X (gfx950) device available: " << selhip_last_error(nullptr) << "\n";
        selhost_dataset_free(db); selhost_dataset_free(qs);
        return 3;
    }
    void* d_out = nullptr;
    selhip_ctx_set_fp_mode(ctx, fp_mode);
    r = selhip_ctx_upload(ctx, selhost_dataset_hll(db), m ? selhost_dataset_aux(db) : no_smh.data(), selhost_dataset_cards(db), n_d, m ? (int)m : 1, 14);
    if (!r && qs) r = selhip_ctx_upload_queries(ctx, selhost_dataset_hll(qs), m ? selhost_dataset_aux(qs) : no_smh.data(), selhost_dataset_cards(qs), n_r);
    if (!r && !values.empty()) r = selhip_malloc(&d_out, values.size() * sizeof(double));
    if (!r) r = qs ? selhip_ctx_query_matrix(ctx, measure, SELHIP_F64, 0, n_r, d_out, n_r, n_d, n_d, row_pos.data(), col_pos.data())
                   : selhip_ctx_matrix(ctx, measure, SELHIP_F64, 0, n_r, d_out, n_r, n_d, n_d, row_pos.data(), col_pos.data());
    if (!r && !values.empty()) r = selhip_memcpy_d2h(values.data(), d_out, values.size() * sizeof(double));
    if (r) std::cerr << "selection: " << selhip_last_error(ctx) << "\n";
    selhip_ctx_destroy(ctx);
    if (d_out) selhip_free(d_out);
    int hr = 0;
    if (!r) {
        hr = selhost_write_matrix(out_file.c_str(), values.data(), n_r, n_d, n_d, row_names.data(), col_names.data());
        if (hr) std::cerr << "selection: " << selhost_last_error() << "\n";
    }
    selhost_dataset_free(db);
    selhost_dataset_free(qs);
    return r ? 4 : hr ? 5 : 0;
}

// a branch length or height as the shortest of %.15g, %.16g, %.17g that reads back to the same double
static std::string newick_number(double x) {
    char buf[64];
    for (int p = 15; p <= 17; ++p) {
        std::snprintf(buf, sizeof buf, "%.*g", p, x);
        if (std::strtod(buf, nullptr) == x) break;
    }
    return buf;
}

// a leaf name: as it is, or in single quotes (a quote doubled) where it is empty or holds a blank or one of ()[]':;,
static std::string newick_name(const std::string& name) {
    if (!name.empty() && name.find_first_of(" ()[]':;,\t\n") == std::string::npos) return name;
    std::string q = "'";
    for (char ch : name) { q += ch; if (ch == '\'') q += ch; }
    return q + "'";
}

// -N / -J: no pass; the hierarchy of the list's dense matrix (selhip_ctx_linkage) as a Newick tree and / or as its merges.
// measure: a symmetric SELHIP_MEASURE_*; m: the SuperMinHash buckets to load for SMH_JACCARD, 0 for the HLL measures
static int run_linkage(const std::string& list_file, int measure, int method, unsigned m, int fp_mode, int threads) {
    selhost_dataset* ds = nullptr;
    if (selhost_dataset_load(&ds, list_file.c_str(), m, 0, fp_mode, threads)) { std::cerr << "selection: -N / -J: " << selhost_last_error() << "\n"; return 1; }
    const int64_t n = selhost_dataset_size(ds);
    const size_t cap = (size_t)std::max<int64_t>(n - 1, 0);
    std::vector<selhip_pair_t> merges(cap);
    std::vector<int32_t> sizes(cap);
    std::vector<uint64_t> no_smh(m ? 0 : (size_t)std::max<int64_t>(1, n), 0);
    selhip_ctx* ctx = nullptr;
    int r = selhip_device_count() > 0 ? selhip_ctx_create(&ctx, 0) : SELHIP_E_NODEVICE;
    if (r) {
        std::cerr << "selection: no MI355X (gfx950) device available: " << selhip_last_error(nullptr) << "\n";
        selhost_dataset_free(ds);
        return 3;
    }
    void* d_merges = nullptr;
    void* d_size = nullptr;
    int64_t f = 0;
    selhip_ctx_set_fp_mode(ctx, fp_mode);
    r = selhip_ctx_upload(ctx, selhost_dataset_hll(ds), m ? selhost_dataset_aux(ds) : no_smh.data(), selhost_dataset_cards(ds), n, m ? (int)m : 1, 14);
    if (!r && cap) r = selhip_malloc(&d_merges, cap * sizeof(selhip_pair_t));
    if (!r && cap) r = selhip_malloc(&d_size, cap * sizeof(int32_t));
    const selhip_linkage_t out{static_cast<selhip_pair_t*>(d_merges), static_cast<int32_t*>(d_size)};
    if (!r) r = selhip_ctx_linkage(ctx, measure, method, INFINITY, &out, &f);
    if (!r && f > 0) r = selhip_memcpy_d2h(merges.data(), d_merges, (size_t)f * sizeof(selhip_pair_t));
    if (!r && f > 0) r = selhip_memcpy_d2h(sizes.data(), d_size, (size_t)f * sizeof(int32_t));
    if (r) std::cerr << "selection: " << selhip_last_error(ctx) << "\n";
    selhip_ctx_destroy(ctx);
    if (d_merges) selhip_free(d_merges);
    if (d_size) selhip_free(d_size);
    int hr = 0;
    if (!r && !g_merges_file.empty()) {
        std::string text;
        for (int64_t s = 0; s < f; ++s)
            text += std::string(selhost_dataset_name(ds, merges[(size_t)s].i)) + "\t" + selhost_dataset_name(ds, merges[(size_t)s].k) + "\t" +
                    std::to_string(merges[(size_t)s].jaccard) + "\t" + std::to_string(sizes[(size_t)s]) + "\n";
        std::ofstream o(g_merges_file, std::ios::binary);
        o << text;
        o.close();
        if (!o) { std::cerr << "selection: -J: cannot write '" << g_merges_file << "'\n"; hr = 5; }
    }
    if (!r && !hr && !g_newick_file.empty()) {
        // nodes 0 .. n - 1 the leaves, n + s the cluster merge s made; root_of[slot] = the node that lives in the slot now
        struct Node { int64_t left, right; double height; };
        std::vector<Node> node((size_t)n + (size_t)f, Node{-1, -1, 0.0});
        std::vector<int64_t> root_of((size_t)std::max<int64_t>(n, 1));
        for (int64_t g = 0; g < n; ++g) root_of[(size_t)g] = g;
        for (int64_t s = 0; s < f; ++s) {
            const selhip_pair_t& e = merges[(size_t)s];
            node[(size_t)(n + s)] = Node{root_of[(size_t)e.i], root_of[(size_t)e.k], e.jaccard};
            root_of[(size_t)e.i] = n + s;
        }
        // written without recursion (a chain is n deep): a stack of nodes to open and of text to emit behind them
        struct Item { int64_t id; double up; bool has_up; std::string text; };
        std::string text;
        std::vector<Item> stack;
        if (n > 0) stack.push_back(Item{root_of[0], 0.0, false, ""});
        while (!stack.empty()) {
            Item it = std::move(stack.back());
            stack.pop_back();
            if (it.id < 0) { text += it.text; continue; }
            const Node& nd = node[(size_t)it.id];
            const std::string tail = it.has_up ? ":" + newick_number(std::max((it.up - nd.height) / 2.0, 0.0)) : "";
            if (nd.left < 0) { text += newick_name(selhost_dataset_name(ds, it.id)) + tail; continue; }
            stack.push_back(Item{-1, 0.0, false, ")" + tail});
            stack.push_back(Item{nd.right, nd.height, true, ""});
            stack.push_back(Item{-1, 0.0, false, ","});
            stack.push_back(Item{nd.left, nd.height, true, ""});
            text += "(";
        }
        text += ";\n";
        std::ofstream o(g_newick_file, std::ios::binary);
        o << text;
        o.close();
        if (!o) { std::cerr << "selection: -N: cannot write '" << g_newick_file << "'\n"; hr = 5; }
    }
    selhost_dataset_free(ds);
    return r ? 4 : hr;
}

// -I ... -P: no pass; the genomes of the list merged by the groups of g_groups_file.  m, p_aux: the sketch files in play, as for a pass
static int run_merge_groups(const std::string& list_file, unsigned m, unsigned p_aux, int fp_mode, int threads) {
    selhost_dataset* ds = nullptr;
    if (selhost_dataset_load(&ds, list_file.c_str(), m, aux_files(p_aux), fp_mode, threads)) { std::cerr << "selection: -P: " << selhost_last_error() << "\n"; return 1; }
    const int64_t n = selhost_dataset_size(ds);
    std::unordered_map<std::string, int64_t> rank_of;
    for (int64_t g = 0; g < n; ++g) rank_of.emplace(selhost_dataset_name(ds, g), g);
    std::vector<int32_t> group((size_t)std::max<int64_t>(n, 1), -1);
    std::vector<std::string> names;
    std::unordered_map<std::string, int32_t> id_of;
    std::ifstream f(g_groups_file, std::ios::binary);
    if (!f) { std::cerr << "selection: -I: cannot read '" << g_groups_file << "'\n"; selhost_dataset_free(ds); return 5; }
    std::string line;
    for (int64_t line_no = 1; std::getline(f, line); ++line_no) {
        if (line.empty()) continue;
        const size_t tab = line.find('\t');
        const std::string gname = tab == std::string::npos ? "" : line.substr(tab + 1);
        const auto it = tab == std::string::npos ? rank_of.end() : rank_of.find(line.substr(0, tab));
        if (it == rank_of.end() || gname.empty() || gname.find('/') != std::string::npos) {
            std::cerr << "selection: -I: line " << line_no << " of '" << g_groups_file
                      << "' is not 'path<TAB>group_name' for a genome of the -l list and a name that is not empty and holds no '/'\n";
            selhost_dataset_free(ds);
            return 5;
        }
        const auto ins = id_of.emplace(gname, (int32_t)names.size());
        if (ins.second) names.push_back(gname);
        group[(size_t)it->second] = ins.first->second;
    }
    std::vector<uint64_t> no_smh(m ? 0 : (size_t)(n > 0 ? n : 1), 0);
    selhip_ctx* ctx = nullptr;
    int r = selhip_device_count() > 0 ? selhip_ctx_create(&ctx, 0) : SELHIP_E_NODEVICE;
    if (r) {
        std::cerr << "selection: no MI355X (gfx950) device available: " << selhip_last_error(nullptr) << "\n";
        selhost_dataset_free(ds);
        return 3;
    }
    selhip_ctx_set_fp_mode(ctx, fp_mode);
    void* d_group = nullptr;
    r = selhip_ctx_upload(ctx, selhost_dataset_hll(ds), m ? selhost_dataset_aux(ds) : no_smh.data(), selhost_dataset_cards(ds), n, m ? (int)m : 1, 14);
    if (!r && p_aux) r = load_aux_hll(ctx, ds, p_aux, false);
    if (!r) r = selhip_malloc(&d_group, group.size() * sizeof(int32_t));
    if (!r) r = selhip_memcpy_h2d(d_group, group.data(), group.size() * sizeof(int32_t));
    if (!r) r = write_merged(ctx, static_cast<const int32_t*>(d_group), (int64_t)names.size(), names);
    if (r && r != 5) std::cerr << "selection: " << selhip_last_error(ctx) << "\n";
    if (d_group) selhip_free(d_group);
    selhip_ctx_destroy(ctx);
    selhost_dataset_free(ds);
    return r == 5 ? 5 : r ? 4 : 0;
}

int main(int argc, char* argv[]) {
    std::string list_file = "";
    float threshold = 0.9f;              // selection_cuda.cpp:62
    int aux_bytes = 256;                 // selection_cuda.cpp:63
    std::string criterion = "smh_a";
    int threads = 8, n_gpus = 1, mode = SELHIP_MODE_CB_SMH, algo = SELHIP_ALGO_AUTO, fp_mode = SELHIP_FP_FMA;
    long long ooc_block = 0;
    std::string out_file = "", dump_file = "", query_file = "", pair_file = "", matrix_file = "", estimator = "", measure_name = "", value_estimator = "";
    bool measure_given = false;
    bool gpus_given = false, topk_given = false, nbr_given = false, matrix_given = false, union_measure = false, aux_given = false, estimator_given = false;
    const char* selection_opt = nullptr;         // the first of -h, -c, -n, -A seen: options of a selection pass, which -M does not run
    long long top_k = 0, nbr_k = 0, min_matches = 0;
    bool cmin_given = false, gamma_given = false, value_given = false, rounds_given = false;
    std::string rounds_arg = "", cluster_min_arg = "", cluster_rep_arg = "";
    bool cluster_given = false, cluster_min_given = false, cluster_rep_given = false, linkage_given = false, priority_given = false;
    std::string linkage_arg = "";
    bool merge_given = false, groups_given = false, forest_given = false;
    bool newick_given = false, merges_given = false, method_given = false;
    std::string method_arg = "";
    int tree_method = SELHIP_LINKAGE_AVERAGE;
    int c;
    while ((c = getopt(argc, argv, "xl:b:a:h:c:C:G:t:g:nA:F:B:o:r:q:k:K:p:M:UE:S:V:R:DL:T:Y:Z:W:P:I:H:N:J:X:")) != -1) {
        switch (c) {
            case 'x': std::cout << "Usage: -l -h -a -b [-c smh_a|hll_a|hll_an|none|smh_c -C c_min|-G gamma] [-t threads] [-g gpus] [-n] [-A auto|stream|sig] [-F 0|1] [-B block] [-o file] | -r file\n"
                                   "       -l db_list -q query_list -h -a [-c smh_a|hll_a|hll_an|none|smh_c -C c_min|-G gamma] [-n] [-A auto|stream|sig|index] [-F 0|1] [-k best_per_query]   (query-vs-database selection)\n"
                                   "       -l -h -a [-c smh_a|hll_a|hll_an|none|smh_c -C c_min|-G gamma] [-n] [-A auto|stream|sig|hashjoin] [-F 0|1] -K best_per_genome   (every genome's best partners, both members of a pair)\n"
                                   "       -l list -p pair_file -h -a [-c smh_a|hll_a|hll_an|none|smh_c -C c_min|-G gamma] [-n] [-A auto|stream|sig] [-F 0|1] [-o file]   (only the listed pairs; lines 'path1 path2 ...')\n"
                                   "       -l list [-q query_list] [-F 0|1] -M out.tsv [-U]   (no selection: the dense Jaccard -- -U: union size -- matrix, file-list order)\n"
                                   "       -l list [-q query_list] -M out.tsv -E smh|smh_matches -a bytes   (the same table from the SuperMinHash sketches: equal buckets / m, or their count)\n"
                                   "       ... -n -S max_containment -h gamma -c smh_c -G gamma -a bytes [-C c_min]   (its prefilter: the count at which the SuperMinHash estimate of the containment is gamma)\n"
                                   "       ... -n -S max_containment [-c smh_a|none|smh_c]   (with -l, -q, -p, -k, -K: select and print I / min(e1, e2), the share of the smaller genome found in the larger)\n"
                                   "       -l list [-q query_list] -M out.tsv -S intersection|containment|max_containment   (the table of I = e1 + e2 - U, I / e_row or I / min(e_row, e_col))\n"
                                   "       ... -c smh_c -C c_min|-G gamma -a bytes -V smh|hll   (with -l, -q, -p, -k, -K, -n, -S max_containment, -o: -V smh tests and prints the SuperMinHash estimate of the count, c / m, with no HLL stage)\n"
                                   "       -l list -K best_per_genome -c smh_c -C c_min|-G gamma -a bytes -V smh -R rows|auto   (the same list in rounds of rows: memory for n K records and one round, not for every pair that shares a bucket)\n"
                                   "       -l list [-p pair_file | -K best_per_genome [-R rows]] ... -L clusters.tsv [-T min_value] [-Y max_degree|min_rank|max_rank]   (besides the output: the single-linkage clusters of the selected pairs, one line per genome: path, cluster, size, degree, representative)\n"
                                   "       ... -L clusters.tsv -Z single|greedy [-T min_value] [-Y max_degree|min_rank|max_rank | -W scores.tsv]   (-Z greedy: greedy representative clusters, CD-HIT style: genomes visited in the -Y order or by descending score, every other genome to its most similar representative; a sixth column: value to the representative)\n"
                                   "       -l list [-p pair_file | -K best_per_genome [-R rows]] ... -H forest.tsv [-T min_value]   (besides the output: the maximum spanning forest of the selected pairs = the merges of the single-linkage dendrogram, one line per edge, best first: path_a, path_b, value; may stand beside -L)\n"
                                   "       -l list -N tree.nwk [-J merges.tsv] [-X average|complete|weighted|single] [-E smh -a bytes | -S max_containment] [-M out.tsv]   (no selection: the hierarchy of the dense matrix under 1 - similarity, on the device: a Newick tree and / or one line per merge: path_a, path_b, height, size)\n"
                                   "       ... -c hll_a|hll_an -a bytes -D   (with -l, -q, -p, -k, -K, -g, -B: no .hll_<p> file is read, the auxiliary HLL sketches are folded from the .hll registers)\n"
                                   "       ... -L clusters.tsv [-Z ...] -P dir   (besides the output: one merged sketch set per cluster in dir -- cluster_<id>.hll, .smh<m>, .hll_<p> -- and dir/filelist.txt, a database for -l)\n"
                                   "       -l list [-c ... -a bytes] -I groups.tsv -P dir   (no selection: the genomes merged by the groups of 'path<TAB>group_name' lines, one sketch set per group_name in dir)\n"; return 0;
            case 'q': query_file = optarg; break;
            case 'p': pair_file = optarg; break;
            case 'M': matrix_file = optarg; matrix_given = true; break;
            case 'U': union_measure = true; break;
            case 'E': estimator = optarg; estimator_given = true; break;
            case 'S': measure_name = optarg; measure_given = true; break;
            case 'V': value_estimator = optarg; value_given = true; break;
            case 'R': rounds_arg = optarg; rounds_given = true; break;
            case 'D': g_fold_aux = true; break;
            case 'L': g_cluster_file = optarg; cluster_given = true; break;
            case 'T': cluster_min_arg = optarg; cluster_min_given = true; break;
            case 'Y': cluster_rep_arg = optarg; cluster_rep_given = true; break;
            case 'Z': linkage_arg = optarg; linkage_given = true; break;
            case 'W': g_priority_file = optarg; priority_given = true; break;
            case 'P': g_merge_dir = optarg; merge_given = true; break;
            case 'H': g_forest_file = optarg; forest_given = true; break;
            case 'N': g_newick_file = optarg; newick_given = true; break;
            case 'J': g_merges_file = optarg; merges_given = true; break;
            case 'X': method_arg = optarg; method_given = true; break;
            case 'I': g_groups_file = optarg; groups_given = true; break;
            case 'k': top_k = std::strtoll(optarg, nullptr, 10); topk_given = true; break;
            case 'K': nbr_k = std::strtoll(optarg, nullptr, 10); nbr_given = true; break;
            case 'B': ooc_block = std::stoll(optarg); break;
            case 'o': out_file = optarg; break;
            case 'r': dump_file = optarg; break;
            case 'l': list_file = optarg; break;
            case 'b': break;
            case 'a': aux_bytes = std::stoi(optarg); aux_given = true; break;
            case 'h': threshold = std::stof(optarg); if (!selection_opt) selection_opt = "-h"; break;
            case 'c': criterion = optarg; if (!selection_opt) selection_opt = "-c"; break;
            case 'C': min_matches = std::strtoll(optarg, nullptr, 10); cmin_given = true; if (!selection_opt) selection_opt = "-C"; break;
            case 'G': g_min_containment = std::strtod(optarg, nullptr); gamma_given = true; if (!selection_opt) selection_opt = "-G"; break;
            case 't': threads = std::stoi(optarg); break;
            case 'g': n_gpus = std::stoi(optarg); gpus_given = true; break;
            case 'n': mode = SELHIP_MODE_SMH; if (!selection_opt) selection_opt = "-n"; break;
            case 'A': if (!selection_opt) selection_opt = "-A"; algo = !strcmp(optarg, "stream") ? SELHIP_ALGO_STREAM : !strcmp(optarg, "sig") ? SELHIP_ALGO_SIG : !strcmp(optarg, "hashjoin") ? SELHIP_ALGO_HASHJOIN : !strcmp(optarg, "index") ? SELHIP_ALGO_INDEX : SELHIP_ALGO_AUTO; break;
            case 'F': fp_mode = std::stoi(optarg) ? SELHIP_FP_FMA : SELHIP_FP_STRICT; break;
            default: break;
        }
    }
    // -N, -J and their -X: checked before any file is read or device opened
    const bool tree_given = newick_given || merges_given;
    if (method_given && !tree_given) { std::cerr << "selection: -X (the linkage method) is an option of -N / -J (the hierarchy of the dense matrix)\n"; return 2; }
    if (tree_given) {
        const char* clash = !query_file.empty() ? "-q" : !pair_file.empty() ? "-p" : gpus_given ? "-g" : ooc_block != 0 ? "-B" : !dump_file.empty() ? "-r"
                          : topk_given ? "-k" : nbr_given ? "-K" : !out_file.empty() ? "-o" : cluster_given ? "-L" : forest_given ? "-H" : merge_given ? "-P"
                          : g_fold_aux ? "-D" : selection_opt;
        if (clash) {
            std::cerr << "selection: -N / -J (the hierarchy of the dense matrix) cannot be combined with " << clash
                      << "; it runs no selection pass, over one list, on one device\n";
            return 2;
        }
        if ((newick_given && g_newick_file.empty()) || (merges_given && g_merges_file.empty())) { std::cerr << "selection: -N / -J need the name of the file to write\n"; return 2; }
        if (method_given) {
            tree_method = method_arg == "single" ? SELHIP_LINKAGE_SINGLE : method_arg == "complete" ? SELHIP_LINKAGE_COMPLETE : method_arg == "average" ? SELHIP_LINKAGE_AVERAGE
                        : method_arg == "weighted" ? SELHIP_LINKAGE_WEIGHTED : -1;
            if (tree_method < 0) { std::cerr << "selection: -X (the linkage method): average, complete, weighted or single, not '" << method_arg << "'\n"; return 2; }
        }
        if (union_measure || (estimator_given && estimator == "smh_matches") || (measure_given && (measure_name == "intersection" || measure_name == "containment"))) {
            std::cerr << "selection: -N / -J take a symmetric similarity: the default (Jaccard), -E smh or -S max_containment; not -U, -E smh_matches, -S intersection | containment\n";
            return 2;
        }
        if (list_file.empty()) { std::cerr << "selection: -N / -J need the list of genomes (-l)\n"; return 2; }
    }
    // -H and its -T: checked before any file is read or device opened
    if (forest_given) {
        const char* clash = !query_file.empty() ? "-q" : matrix_given ? "-M" : gpus_given ? "-g" : ooc_block != 0 ? "-B" : !dump_file.empty() ? "-r" : nullptr;
        if (clash) {
            std::cerr << "selection: -H (the spanning forest of the selected pairs) cannot be combined with " << clash
                      << "; it takes the result list one all-pairs or pair-list pass leaves on one device\n";
            return 2;
        }
        if (g_forest_file.empty()) { std::cerr << "selection: -H needs the name of the file to write\n"; return 2; }
        if (cluster_min_given && !cluster_given) {                       // (beside -L the one -T serves both and is read there)
            char* end = nullptr;
            g_cluster_min = std::strtod(cluster_min_arg.c_str(), &end);
            if (cluster_min_arg.empty() || *end || std::isnan(g_cluster_min)) {
                std::cerr << "selection: -T (with -H: the smallest value of an edge) must be a number, not '" << cluster_min_arg << "'\n";
                return 2;
            }
        }
    }
    // -L and its -T, -Y: checked before any file is read or device opened
    if (((cluster_min_given && !forest_given) || cluster_rep_given) && !cluster_given) {
        std::cerr << "selection: " << (cluster_min_given && !forest_given ? "-T (the smallest value of an edge)" : "-Y (the representative of a cluster)")
                  << " is an option of -L (the clusters of the selected pairs)\n";
        return 2;
    }
    // -Z and -W: checked before any file is read or device opened
    if ((linkage_given || priority_given) && !cluster_given) {
        std::cerr << "selection: " << (linkage_given ? "-Z (single or greedy clusters)" : "-W (the scores that order the greedy clusters)")
                  << " is an option of -L (the clusters of the selected pairs)\n";
        return 2;
    }
    if (linkage_given) {
        if (linkage_arg == "greedy") g_cluster_greedy = true;
        else if (linkage_arg != "single") {
            std::cerr << "selection: -Z (with -L: how the selected pairs are clustered): single or greedy, not '" << linkage_arg << "'\n";
            return 2;
        }
    }
    if (priority_given) {
        if (!g_cluster_greedy) {
            std::cerr << "selection: -W (the scores that order the greedy clusters) is an option of -L ... -Z greedy\n";
            return 2;
        }
        if (cluster_rep_given) {
            std::cerr << "selection: -W (the scores that order the greedy clusters of -L) cannot be combined with -Y; the scores are the order\n";
            return 2;
        }
        if (g_priority_file.empty()) { std::cerr << "selection: -W (with -L -Z greedy) needs the name of the file of scores\n"; return 2; }
    }
    // -P and -I: checked before any file is read or device opened
    if (groups_given && !merge_given) { std::cerr << "selection: -I (the groups file) is an option of -P (one merged sketch set per group)\n"; return 2; }
    if (merge_given) {
        if (!cluster_given && !groups_given) {
            std::cerr << "selection: -P (one merged sketch set per group) needs its groups: -L (the clusters of the selected pairs) or -I (a groups file)\n";
            return 2;
        }
        if (cluster_given && groups_given) { std::cerr << "selection: -I (the groups file of -P) cannot be combined with -L; the groups are the one or the other\n"; return 2; }
        const char* clash = !query_file.empty() ? "-q" : matrix_given ? "-M" : gpus_given ? "-g" : ooc_block != 0 ? "-B" : !dump_file.empty() ? "-r" : nullptr;
        if (clash) {
            std::cerr << "selection: -P (one merged sketch set per group) cannot be combined with " << clash
                      << "; it merges the sketches one context holds on one device\n";
            return 2;
        }
        const char* pass = !groups_given ? nullptr : !pair_file.empty() ? "-p" : topk_given ? "-k" : nbr_given ? "-K" : !out_file.empty() ? "-o" : nullptr;
        if (pass) { std::cerr << "selection: -I (the groups file of -P) cannot be combined with " << pass << "; it runs no selection pass\n"; return 2; }
        if (g_merge_dir.empty()) { std::cerr << "selection: -P needs the name of the directory to write\n"; return 2; }
        if (groups_given && g_groups_file.empty()) { std::cerr << "selection: -I needs the name of the groups file\n"; return 2; }
    }
    if (cluster_given) {
        const char* clash = !query_file.empty() ? "-q" : matrix_given ? "-M" : gpus_given ? "-g" : ooc_block != 0 ? "-B" : !dump_file.empty() ? "-r" : nullptr;
        if (clash) {
            std::cerr << "selection: -L (the clusters of the selected pairs) cannot be combined with " << clash
                      << "; it clusters the result list one all-pairs or pair-list pass leaves on one device\n";
            return 2;
        }
        if (g_cluster_file.empty()) { std::cerr << "selection: -L needs the name of the file to write\n"; return 2; }
        if (cluster_min_given) {
            char* end = nullptr;
            g_cluster_min = std::strtod(cluster_min_arg.c_str(), &end);
            if (cluster_min_arg.empty() || *end || std::isnan(g_cluster_min)) {
                std::cerr << "selection: -T (with -L: the smallest value of an edge) must be a number, not '" << cluster_min_arg << "'\n";
                return 2;
            }
        }
        if (cluster_rep_given) {
            if (cluster_rep_arg == "max_degree") g_cluster_rep = SELHIP_REP_MAX_DEGREE;
            else if (cluster_rep_arg == "min_rank") g_cluster_rep = SELHIP_REP_MIN_RANK;
            else if (cluster_rep_arg == "max_rank") g_cluster_rep = SELHIP_REP_MAX_RANK;
            else {
                std::cerr << "selection: -Y (with -L: the representative of a cluster): max_degree, min_rank or max_rank, not '" << cluster_rep_arg << "'\n";
                return 2;
            }
        }
    }
    // -D: checked before any file is read or device opened
    if (g_fold_aux) {
        if (matrix_given) { std::cerr << "selection: -D (fold the auxiliary HLL sketches) cannot be combined with -M; the dense similarity matrix reads no auxiliary sketch\n"; return 2; }
        if (!dump_file.empty()) { std::cerr << "selection: -D (fold the auxiliary HLL sketches) cannot be combined with -r; printing a result file reads no sketch\n"; return 2; }
        if (criterion != "hll_a" && criterion != "hll_an") {
            std::cerr << "selection: -D folds the auxiliary HLL sketches of -c hll_a | hll_an; -c " << criterion << " reads none\n";
            return 2;
        }
        const int p_fold = __builtin_ctz(aux_bytes ? aux_bytes : 1);
        if (p_fold < 4 || p_fold > 14) {
            std::cerr << "selection: -D: the auxiliary precision ctz(-a " << aux_bytes << ") = " << p_fold << " must be in 4..14 (the .hll registers have p = 14)\n";
            return 2;
        }
    }
    // -V: checked before any file is read or device opened
    if (value_given) {
        if (value_estimator != "hll" && value_estimator != "smh") {
            std::cerr << "selection: -V (the estimator of a selection pass): hll or smh, not '" << value_estimator << "'\n";
            return 2;
        }
        if (value_estimator == "smh") {
            if (matrix_given) { std::cerr << "selection: -V smh is an option of a selection pass; the estimator of -M (the dense similarity matrix) is -E\n"; return 2; }
            if (criterion != "smh_c") {
                std::cerr << "selection: -V smh needs -c smh_c: the SuperMinHash estimate is computed from the count of equal buckets, which that criterion alone takes\n";
                return 2;
            }
            const char* clash = gpus_given ? "-g" : ooc_block != 0 ? "-B" : nullptr;
            if (clash) {
                std::cerr << "selection: -V smh cannot be combined with " << clash << "; the multi-GPU and out-of-core drivers carry no estimator\n";
                return 2;
            }
            g_estimator = SELHIP_ESTIMATOR_SMH;
        }
    }
    // -R: checked before any file is read or device opened
    if (rounds_given) {
        const char* clash = !query_file.empty() ? "-q" : !pair_file.empty() ? "-p" : matrix_given ? "-M" : gpus_given ? "-g" : ooc_block != 0 ? "-B" : nullptr;
        if (clash) {
            std::cerr << "selection: -R (the rows per round of -K) cannot be combined with " << clash << "; it cuts one all-pairs pass on one device into rounds\n";
            return 2;
        }
        if (!nbr_given) { std::cerr << "selection: -R (the rows per round) is an option of -K (the best partners of every genome)\n"; return 2; }
        if (criterion != "smh_c" || g_estimator != SELHIP_ESTIMATOR_SMH) {
            std::cerr << "selection: -R needs -c smh_c -V smh: the rounds prune with the value the count kernel computes\n";
            return 2;
        }
        char* end = nullptr;
        g_topk_rounds = rounds_arg == "auto" ? SELHIP_TOPK_ROUNDS_AUTO : std::strtoll(rounds_arg.c_str(), &end, 10);
        if (rounds_arg != "auto" && (rounds_arg.empty() || *end || g_topk_rounds < 1)) {
            std::cerr << "selection: -R must be a number of rows >= 1 or auto, not '" << rounds_arg << "'\n";
            return 2;
        }
    }
    // -S: checked before any file is read or device opened
    int pass_measure = SELHIP_MEASURE_JACCARD, matrix_measure = SELHIP_MEASURE_JACCARD;
    if (measure_given) {
        const bool matrix_only = measure_name == "intersection" || measure_name == "containment";
        if (measure_name != "jaccard" && measure_name != "max_containment" && !matrix_only) {
            std::cerr << "selection: -S (the measure): jaccard or max_containment, with -M also intersection or containment, not '" << measure_name << "'\n";
            return 2;
        }
        if (matrix_only && !matrix_given && !tree_given) {
            std::cerr << "selection: -S " << measure_name << " is a measure of -M (the dense similarity matrix); a selection pass takes -S jaccard or -S max_containment\n";
            return 2;
        }
        matrix_measure = measure_name == "intersection" ? SELHIP_MEASURE_INTERSECTION : measure_name == "containment" ? SELHIP_MEASURE_CONTAINMENT
                       : measure_name == "max_containment" ? SELHIP_MEASURE_MAX_CONTAINMENT : SELHIP_MEASURE_JACCARD;
        if (union_measure) { std::cerr << "selection: -S (the measure) cannot be combined with -U: the union size is a measure of its own\n"; return 2; }
        if (estimator_given && estimator != "hll") {
            std::cerr << "selection: -S (a measure from the HyperLogLog sketches) cannot be combined with -E " << estimator << "\n";
            return 2;
        }
        if (!matrix_given && !tree_given && measure_name == "max_containment") {
            pass_measure = SELHIP_MEASURE_MAX_CONTAINMENT;
            if (mode != SELHIP_MODE_SMH) {
                std::cerr << "selection: -S max_containment needs -n: the CB bound is a bound on J and cuts the pairs of unequal size the measure exists for\n";
                return 2;
            }
            if (criterion == "hll_a" || criterion == "hll_an") {
                std::cerr << "selection: -S max_containment cannot be combined with -c " << criterion << ": its bound is derived for J (use -c smh_a, none or smh_c)\n";
                return 2;
            }
            const char* clash = gpus_given ? "-g" : ooc_block != 0 ? "-B" : !out_file.empty() ? "-o" : nullptr;
            if (clash) {
                std::cerr << "selection: -S max_containment cannot be combined with " << clash
                          << "; the multi-GPU and out-of-core drivers carry no measure and the result file records none\n";
                return 2;
            }
        }
    }
    if (matrix_given || tree_given) {
        // checked before any file is read or device opened
        const char* clash = !matrix_given ? nullptr : !pair_file.empty() ? "-p" : topk_given ? "-k" : nbr_given ? "-K" : gpus_given ? "-g" : ooc_block != 0 ? "-B"
                          : !out_file.empty() ? "-o" : !dump_file.empty() ? "-r" : selection_opt;
        if (clash) {
            std::cerr << "selection: -M (the dense similarity matrix) cannot be combined with " << clash
                      << "; it runs no selection pass (no criterion, threshold, CB bound or algorithm), on one device, and writes a table\n";
            return 2;
        }
        if (list_file.empty()) { std::cerr << "selection: -M needs the list of genomes (-l)\n"; return 2; }
        int measure = union_measure ? SELHIP_MEASURE_UNION : matrix_measure;
        unsigned m_smh = 0;
        if (estimator_given && estimator != "hll") {
            if (estimator != "smh" && estimator != "smh_matches") {
                std::cerr << "selection: -E (the estimator of -M): hll, smh or smh_matches, not '" << estimator << "'\n";
                return 2;
            }
            if (union_measure) { std::cerr << "selection: -U (union sizes) is a value of -E hll; -E " << estimator << " has no union size\n"; return 2; }
            if (!aux_given || aux_bytes / 8 <= 0) {
                std::cerr << "selection: -E " << estimator << " reads the .smh<m> files: give their size with -a (bytes, 8 per bucket)\n";
                return 2;
            }
            measure = estimator == "smh" ? SELHIP_MEASURE_SMH_JACCARD : SELHIP_MEASURE_SMH_MATCHES;
            m_smh = (unsigned)aux_bytes / 8;
        }
        int rc = matrix_given ? run_matrix(list_file, query_file, matrix_file, measure, m_smh, fp_mode, threads) : 0;
        if (!rc && tree_given) rc = run_linkage(list_file, measure, tree_method, m_smh, fp_mode, threads);
        return rc;
    }
    if (estimator_given) { std::cerr << "selection: -E (hll, smh, smh_matches) is an option of -M (the dense similarity matrix)\n"; return 2; }
    if (union_measure) { std::cerr << "selection: -U (union sizes) is an option of -M (the dense similarity matrix)\n"; return 2; }
    // -c smh_c and its -C: checked before any file is read or device opened
    if (cmin_given && criterion != "smh_c") { std::cerr << "selection: -C (the count threshold) is an option of -c smh_c\n"; return 2; }
    if (gamma_given && criterion != "smh_c") { std::cerr << "selection: -G (the minimum containment) is an option of -c smh_c\n"; return 2; }
    if (gamma_given && !std::isfinite(g_min_containment)) { std::cerr << "selection: -G must be a finite number\n"; return 2; }
    if (criterion == "smh_c") {
        if (!cmin_given && !gamma_given) { std::cerr << "selection: -c smh_c needs its count threshold: -C c_min (at least c_min equal buckets)\n"; return 2; }
        if (!aux_given || aux_bytes / 8 <= 0) { std::cerr << "selection: -c smh_c reads the .smh<m> files: give their size with -a (bytes, 8 per bucket)\n"; return 2; }
        const char* clash = gpus_given ? "-g" : ooc_block != 0 ? "-B" : nullptr;
        if (clash) {
            std::cerr << "selection: -c smh_c cannot be combined with " << clash << "; the multi-GPU and out-of-core drivers carry no count threshold\n";
            return 2;
        }
        if (cmin_given && (min_matches < 1 || min_matches > aux_bytes / 8)) { std::cerr << "selection: -C must be in 1.." << aux_bytes / 8 << " (the m = -a / 8 buckets)\n"; return 2; }
    }
    if (!pair_file.empty()) {
        // checked before any file is read or device opened
        const char* clash = !query_file.empty() ? "-q" : topk_given ? "-k" : nbr_given ? "-K" : ooc_block != 0 ? "-B" : gpus_given && n_gpus > 1 ? "-g" : nullptr;
        if (clash) {
            std::cerr << "selection: -p (selection over a list of pairs) cannot be combined with " << clash
                      << "; it runs one pass over the listed pairs on one device\n";
            return 2;
        }
    }
    if (topk_given) {
        // checked before any file is read or device opened
        if (query_file.empty()) { std::cerr << "selection: -k (the best pairs per query) needs -q (the query list)\n"; return 2; }
        if (top_k < 1 || top_k > SELHIP_TOPK_MAX) { std::cerr << "selection: -k must be in 1.." << SELHIP_TOPK_MAX << "\n"; return 2; }
    }
    if (nbr_given) {
        // checked before any file is read or device opened
        if (!query_file.empty()) {
            std::cerr << "selection: -K (the best partners of every genome of one list) cannot be combined with -q; the best pairs per query are -k\n";
            return 2;
        }
        const char* clash = gpus_given ? "-g" : ooc_block != 0 ? "-B" : !out_file.empty() ? "-o" : !dump_file.empty() ? "-r" : nullptr;
        if (clash) {
            std::cerr << "selection: -K (the best partners of every genome) cannot be combined with " << clash
                      << "; it runs on one device and prints text\n";
            return 2;
        }
        if (nbr_k < 1 || nbr_k > SELHIP_TOPK_MAX) { std::cerr << "selection: -K must be in 1.." << SELHIP_TOPK_MAX << "\n"; return 2; }
    }
    if (!query_file.empty()) {
        // checked before any file is read or device opened
        const char* clash = gpus_given ? "-g" : ooc_block != 0 ? "-B" : !out_file.empty() ? "-o" : !dump_file.empty() ? "-r" : nullptr;
        if (clash) {
            std::cerr << "selection: -q (query-vs-database selection) cannot be combined with " << clash
                      << "; it runs on one device and prints text\n";
            return 2;
        }
        if (criterion != "smh_a" && criterion != "hll_a" && criterion != "hll_an" && criterion != "none" && criterion != "smh_c") {
            std::cerr << "selection: -q -c " << criterion << ": the accepted criteria are hll_a, hll_an and smh_a\n";
            return 2;
        }
        if (list_file.empty()) { std::cerr << "selection: -q needs the database list (-l)\n"; return 2; }
        return run_queries(query_file, list_file, criterion, threshold, aux_bytes, mode, algo, fp_mode, threads, (int)top_k, (int)min_matches, pass_measure);
    }
    if (algo == SELHIP_ALGO_INDEX) {
        // checked before any file is read or device opened
        std::cerr << "selection: -A index is an algorithm of query-vs-database selection: it needs -q (the query list)\n";
        return 2;
    }
    if (!dump_file.empty()) {
        selhost_results* res = nullptr;
        if (selhost_read_results(&res, dump_file.c_str())) { std::cerr << "selection: " << selhost_last_error() << "\n"; return 5; }
        const int64_t need = selhost_results_text(res, nullptr, 0);
        if (need < 0) { std::cerr << "selection: " << selhost_last_error() << "\n"; selhost_results_free(res); return 5; }
        std::string text((size_t)need + 1, '\0');
        selhost_results_text(res, &text[0], text.size());
        text.resize((size_t)need);
        std::cout << text;
        selhost_results_free(res);
        return 0;
    }
    int crit = SELHIP_CRIT_SMH_A;
    if (criterion == "hll_a") crit = SELHIP_CRIT_HLL_A;
    else if (criterion == "hll_an") crit = SELHIP_CRIT_HLL_AN;
    else if (criterion == "none") crit = SELHIP_CRIT_NONE;
    else if (criterion == "smh_c") crit = SELHIP_CRIT_SMH_C;
    else if (criterion != "smh_a") {
        std::cout << "Option -c invalid. The accepted criteria are hll_a, hll_an and smh_a.\n";    // selection.cpp:293
        return 0;
    }
    if (list_file.empty()) { std::cerr << "No input file provided\n"; exit(-1); }   // selection.cpp:40-44
    if (nbr_given) return run_neighbours(list_file, crit, threshold, aux_bytes, mode, algo, fp_mode, threads, (int)nbr_k, (int)min_matches, pass_measure);
    const bool reads_smh = crit == SELHIP_CRIT_SMH_A || crit == SELHIP_CRIT_SMH_C;
    const unsigned m = reads_smh ? (unsigned)aux_bytes / 8 : 0;                                      // selection.cpp:231
    const unsigned p_aux = reads_smh || crit == SELHIP_CRIT_NONE ? 0 : (unsigned)__builtin_ctz(aux_bytes ? aux_bytes : 1);   // :125
    g_merge_m = m; g_merge_p_aux = p_aux;
    if (groups_given) return run_merge_groups(list_file, m, p_aux, fp_mode, threads);

    selhost_dataset* ds = nullptr;
    int rc = selhost_dataset_load(&ds, list_file.c_str(), m, aux_files(p_aux), fp_mode, threads);
    if (rc) { std::cerr << selhost_last_error() << "\n"; exit(-1); }
    const int64_t n = selhost_dataset_size(ds);
    if (const int w = load_priorities(ds, n)) return w;
    // the auxiliary HLL array of the drivers that take host arrays (-B, -g): the files', or under -D the host fold of the .hll registers
    std::vector<uint8_t> folded;
    const uint8_t* aux_hll_host = p_aux ? selhost_dataset_aux_hll(ds) : nullptr;
    if (g_fold_aux && p_aux && (ooc_block > 0 || n_gpus > 1)) {
        folded.resize(std::max<size_t>(1, (size_t)n << p_aux));
        if (selhost_hll_fold(selhost_dataset_hll(ds), n, 14, p_aux, folded.data())) { std::cerr << "selection: -D: " << selhost_last_error() << "\n"; return 5; }
        aux_hll_host = folded.data();
    }

    int n_rows = 1, n_bands = 1;
    if (m) selhost_banding(m, threshold, SELHOST_BANDING_CPU, &n_rows, &n_bands);
    // hll_a / hll_an do not read SuperMinHash buckets: a one-bucket placeholder keeps the upload call uniform
    std::vector<uint64_t> no_smh(m ? 0 : (size_t)(n > 0 ? n : 1), 0);
    const uint64_t* aux_ptr = m ? selhost_dataset_aux(ds) : no_smh.data();
    const int m_up = m ? (int)m : 1;

    const int avail = selhip_device_count();
    if (avail <= 0) { std::cerr << "selection: no MI355X (gfx950) device available: " << selhip_last_error(nullptr) << "\n"; return 3; }
    if (n_gpus < 1) n_gpus = 1;
    if (n_gpus > avail) n_gpus = avail;

    std::vector<std::vector<selhip_pair_t>> parts(1);
    if (ooc_block > 0) {
        // sketches stay in host memory; block pairs are uploaded in turn (two at a time: upload overlaps compute)
        int64_t cnt = 0, cap = 1 << 20;
        for (int attempt = 0; attempt < 2; ++attempt) {
            parts[0].resize((size_t)cap);
            int r = selhip_ooc_select(0, selhost_dataset_hll(ds), aux_ptr, selhost_dataset_cards(ds),
                                      aux_hll_host, (int)p_aux, crit, n, m_up, 14,
                                      mode, algo, fp_mode, threshold, n_rows, n_bands, ooc_block, 2, parts[0].data(), cap, &cnt, nullptr);
            if (r == SELHIP_E_OVERFLOW && attempt == 0) { cap = cnt; continue; }
            if (r) { std::cerr << "selection: " << selhip_last_error(nullptr) << "\n"; return 4; }
            break;
        }
        parts[0].resize((size_t)cnt);
        n_gpus = 1;
    } else if (n_gpus > 1) {
        // one process, one thread + context per device, selected pairs gathered over RCCL/xGMI (host merge if RCCL is
        // unavailable): selhip_multi_select
        std::vector<int> devs((size_t)n_gpus);
        for (int g = 0; g < n_gpus; ++g) devs[(size_t)g] = g;
        int64_t cnt = 0, cap = 1 << 20;
        for (int attempt = 0; attempt < 2; ++attempt) {
            parts[0].resize((size_t)cap);
            int r = selhip_multi_select(devs.data(), n_gpus, selhost_dataset_hll(ds), aux_ptr, selhost_dataset_cards(ds),
                                        aux_hll_host, (int)p_aux, crit, n, m_up, 14,
                                        mode, algo, fp_mode, threshold, n_rows, n_bands, SELHIP_GATHER_RCCL_OR_HOST,
                                        parts[0].data(), cap, &cnt, nullptr);
            if (r == SELHIP_E_OVERFLOW && attempt == 0) { cap = cnt; continue; }
            if (r) { std::cerr << "selection: " << selhip_last_error(nullptr) << "\n"; return 4; }
            break;
        }
        parts[0].resize((size_t)cnt);
        n_gpus = 1;                                   // one merged, sorted part
    } else {
        n_gpus = 1;
        selhip_ctx* ctx = nullptr;
        int r = selhip_ctx_create(&ctx, 0);
        if (r) { std::cerr << "selection: " << selhip_last_error(nullptr) << "\n"; return 4; }
        selhip_ctx_set_fp_mode(ctx, fp_mode);
        r = selhip_ctx_upload(ctx, selhost_dataset_hll(ds), aux_ptr, selhost_dataset_cards(ds), n, m_up, 14);
        if (!r && p_aux) r = load_aux_hll(ctx, ds, p_aux, false);
        if (!r) r = selhip_ctx_set_criterion(ctx, crit);
        if (!r && crit == SELHIP_CRIT_SMH_C) r = set_count_thresholds(ctx, (int)min_matches);
        if (!r) r = selhip_ctx_set_measure(ctx, pass_measure);
        void* d_list = nullptr;
        if (!r && !pair_file.empty()) {
            // the listed pairs as ranks of the sorted list, then one pass over them
            std::vector<const char*> names((size_t)n);
            for (int64_t g = 0; g < n; ++g) names[(size_t)g] = selhost_dataset_name(ds, g);
            std::vector<int32_t> xy;
            int64_t cnt = 0;
            int hr = selhost_read_pair_list(pair_file.c_str(), names.data(), n, nullptr, 0, &cnt);
            if (!hr) { xy.resize((size_t)cnt * 2); hr = selhost_read_pair_list(pair_file.c_str(), names.data(), n, xy.data(), cnt, &cnt); }
            if (hr) { std::cerr << "selection: " << selhost_last_error() << "\n"; selhip_ctx_destroy(ctx); return 5; }
            if (cnt > 0x7FFFFFFFll) { std::cerr << "selection: more than 2^31 - 1 pairs in " << pair_file << "\n"; selhip_ctx_destroy(ctx); return 5; }
            if (cnt) r = selhip_malloc(&d_list, (size_t)cnt * 8);
            if (!r && cnt) r = selhip_memcpy_h2d(d_list, xy.data(), (size_t)cnt * 8);
            if (!r) r = selhip_ctx_run_pairs(ctx, static_cast<const selhip_int2_t*>(d_list), cnt, mode, algo, threshold, n_rows, n_bands);
        } else if (!r) {
            r = selhip_ctx_run(ctx, mode, algo, threshold, n_rows, n_bands, 0, n);
        }
        if (!r) {
            int64_t cnt = selhip_ctx_result_count(ctx);
            parts[0].resize((size_t)cnt);
            r = selhip_ctx_fetch(ctx, parts[0].data(), cnt);
        }
        if (!r) r = write_clusters(ctx, ds, n);
        if (r) { std::cerr << "selection: " << selhip_last_error(ctx) << "\n"; selhip_ctx_destroy(ctx); return 4; }
        selhip_ctx_destroy(ctx);
        if (d_list) selhip_free(d_list);
    }

    if (!out_file.empty()) {
        std::vector<const char*> names((size_t)n);
        for (int64_t g = 0; g < n; ++g) names[(size_t)g] = selhost_dataset_name(ds, g);
        static_assert(sizeof(selhost_pair_t) == sizeof(selhip_pair_t), "record layouts must agree");
        const int r = selhost_write_results(out_file.c_str(), reinterpret_cast<const selhost_pair_t*>(parts[0].data()), (int64_t)parts[0].size(),
                                            names.data(), n, threshold);
        if (r) { std::cerr << "selection: " << selhost_last_error() << "\n"; return 5; }
        selhost_dataset_free(ds);
        return 0;
    }
    // shards are contiguous row ranges and each part is sorted by (i,k): concatenation = print order
    std::string out;
    char line[8192];
    for (int g = 0; g < n_gpus; ++g)
        for (const selhip_pair_t& pr : parts[(size_t)g]) {
            int w = selhost_format_line(selhost_dataset_name(ds, pr.i), selhost_dataset_name(ds, pr.k), pr.jaccard, line, sizeof line);
            if (w > 0) out.append(line, (size_t)w);
        }
    std::cout << out;
    selhost_dataset_free(ds);
    return 0;
}
