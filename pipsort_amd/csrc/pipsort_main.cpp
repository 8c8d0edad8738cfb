// pipsort_main.cpp — the PIPSORT command line, drop-in for the reference
// driver (pipsort.cpp:68-228 + Model, model.h:60-310), with PostCal replaced
// by the MI355X engine behind include/pipsort_engine.h.
//
// Same options (optstring of pipsort.cpp:90, including its quirks: -m falls
// through into -n, options without an argument abort with "optarg is NULL"),
// same input formats and the same output files.
#include <fcntl.h>
#include <sched.h>
#include <getopt.h>
#include <thread>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../include/pipsort_engine.h"
#include "../../include/pipsort_model.h"

using std::string;
using std::vector;

namespace {

// pipsort.cpp:28-44
vector<string> read_dir(const string& fn) {
    vector<string> dirs;
    std::ifstream fin(fn.c_str());
    if (!fin) {
        std::cout << "Error: unable to open " << fn << std::endl;
        exit(1);
    }
    string line;
    while (fin.good()) {
        std::getline(fin, line);
        if (line != "") dirs.push_back(line);
    }
    return dirs;
}

// pipsort.cpp:46-66
vector<int> read_sigma(const string& s) {
    vector<int> sizes;
    string cur = "";
    for (char ch : s) {
        if (ch == ',') {
            sizes.push_back((int)std::stod(cur));
            cur = "";
        } else if (isdigit((unsigned char)ch)) {
            cur += ch;
        } else {
            std::cout << "Error: sample size is not in the right format" << std::endl;
            exit(1);
        }
    }
    if (cur != "") sizes.push_back((int)std::stod(cur));
    return sizes;
}

// util.cpp:86-96 importData: doubles separated by whitespace, stopping at the
// first token `istream >> double` would reject.  mmap + strtod, parsed in
// parallel chunks cut at whitespace: each chunk parses until its own first
// rejected token, and the result is the chunks in order up to the first chunk
// that stopped — exactly the sequential parse (an M = 2000 LD file is 150 MB).
namespace {
struct ParsedChunk {
    vector<double> v;
    bool stopped = false;
};

// One `istream >> double` extraction (libstdc++ num_get::_M_extract_float +
// __convert_to_v): an optional sign, digits with at most one '.', then - after
// at least one digit - an 'e'/'E' with an optional sign and digits; the
// collected characters must convert completely and finitely ("1e400", "-nan",
// "inf", "1e+" fail; "0x10" yields 0 and stops at 'x').  Returns the end of
// the characters consumed, or nullptr when the extraction fails.
const char* extract_double(const char* s, const char* end, double& v) {
    char buf[512];
    size_t n = 0;
    const char* p = s;
    auto put = [&](char c) {
        if (n + 1 < sizeof(buf)) buf[n++] = c;
    };
    if (p < end && (*p == '+' || *p == '-')) put(*p++);
    bool mant = false, dec = false, sci = false;
    while (p < end) {
        const char c = *p;
        if (isdigit((unsigned char)c)) {
            put(c);
            mant = true;
        } else if (c == '.' && !dec && !sci) {
            put('.');
            dec = true;
        } else if ((c == 'e' || c == 'E') && !sci && mant) {
            put('e');
            sci = true;
            if (p + 1 < end && (p[1] == '+' || p[1] == '-')) put(*++p);
        } else {
            break;
        }
        p++;
    }
    if (n + 1 >= sizeof(buf)) return nullptr;  // a 500-character number: not an LD entry
    buf[n] = 0;
    char* e = nullptr;
    v = strtod(buf, &e);
    if (e == buf || *e != 0 || std::isinf(v)) return nullptr;
    return p;
}

// host threads this process may run on (its CPU affinity set)
unsigned affinity_cores() {
    cpu_set_t set;
    CPU_ZERO(&set);
    if (sched_getaffinity(0, sizeof(set), &set) == 0) return std::max(1, CPU_COUNT(&set));
    return std::max(1u, std::thread::hardware_concurrency());
}

void parse_chunk(const char* s, const char* end, ParsedChunk& out) {
    // a thread-local vector, moved out at the end: the chunks' vector headers sit
    // side by side in one array, and pushing into them per token would make the
    // threads share their cache lines
    vector<double> vals;
    vals.reserve((size_t)(end - s) / 8 + 1);
    bool stopped = false;
    while (s < end) {
        while (s < end && isspace((unsigned char)*s)) s++;
        if (s >= end) break;
        double v = 0;
        const char* e = extract_double(s, end, v);
        if (!e) { stopped = true; break; }
        vals.push_back(v);
        s = e;
    }
    out.v = std::move(vals);
    out.stopped = stopped;
}
}  // namespace

bool import_data(const string& fn, vector<double>& out) {
    int fd = open(fn.c_str(), O_RDONLY);
    if (fd < 0) {
        std::cout << "Unable to open file; This is why";
        return false;
    }
    struct stat st;
    fstat(fd, &st);
    size_t len = (size_t)st.st_size;
    if (len == 0) { close(fd); return true; }
    char* p = (char*)mmap(nullptr, len + 1, PROT_READ, MAP_PRIVATE, fd, 0);
    close(fd);
    if (p == MAP_FAILED) return false;
    string buf(p, len);  // NUL-terminated copy for strtod
    munmap(p, len + 1);
    const char* s = buf.c_str();
    const char* end = s + len;
    // every core of the affinity set, but at least 512 KB of text per thread
    const size_t nt = std::max<size_t>(1, std::min<size_t>(affinity_cores(), len >> 19));
    // chunk boundaries at whitespace, so no token is split
    vector<const char*> cut(nt + 1);
    cut[0] = s;
    cut[nt] = end;
    for (size_t i = 1; i < nt; i++) {
        const char* c = s + len * i / nt;
        if (c < cut[i - 1]) c = cut[i - 1];
        while (c < end && !isspace((unsigned char)*c)) c++;
        cut[i] = c;
    }
    vector<ParsedChunk> parts(nt);
    vector<std::thread> th;
    for (size_t i = 1; i < nt; i++) th.emplace_back(parse_chunk, cut[i], cut[i + 1], std::ref(parts[i]));
    parse_chunk(cut[0], cut[1], parts[0]);
    for (auto& t : th) t.join();
    size_t total = 0;
    for (auto& c : parts) total += c.v.size();
    out.reserve(out.size() + total);
    for (auto& c : parts) {
        out.insert(out.end(), c.v.begin(), c.v.end());
        if (c.stopped) break;
    }
    return true;
}

// util.cpp:132-159 (first column names, second column z)
void import_z(const string& fn, vector<string>& names, vector<double>& z) {
    std::ifstream fin(fn.c_str());
    string line, first = "", second;
    double d = 0.0;
    while (std::getline(fin, line)) {
        std::istringstream a(line);
        a >> first;
        names.push_back(first);
        std::istringstream b(line);
        b >> second;
        b >> d;
        z.push_back(d);
    }
}

// util.cpp:99-126
bool import_snp_map(const string& fn, int ncols, vector<string>& first, vector<vector<int>>& rest) {
    std::ifstream f(fn.c_str());
    if (!f.is_open()) {
        std::cout << "Could not open file\n";
        return false;
    }
    string line, word;
    while (std::getline(f, line)) {
        std::stringstream s(line);
        for (int i = 0; i < ncols; i++) {
            std::getline(s, word, ',');
            if (i == 0) first.push_back(word);
            else rest[i - 1].push_back(std::stoi(word));
        }
    }
    return true;
}

double special_exp(double post, double total) { return post == 0 ? 0 : std::exp(post - total); }  // postcal.h:277-283

bool g_multi = false;  // several devices: errors come from the psx_multi layer

// Phase timing of one run (PSX_TIMING=1: one "psx-timing {json}" line on
// stderr at exit).  Wall-clock epoch milliseconds, so a parent that records its
// own time before spawning the process (PSX_T0 = epoch ns) sees process start
// + dynamic loading as the gap to main.
double epoch_ms() {
    return std::chrono::duration<double, std::milli>(std::chrono::system_clock::now().time_since_epoch()).count();
}
struct PhaseTimes {
    double main = 0, parse0 = 0, parse1 = 0, rt0 = 0, rt1 = 0, warm1 = 0, joined = 0, setup1 = 0, sweep1 = 0,
           accum1 = 0, write1 = 0, end = 0;
} g_ph;
psx_setup_info g_setup_info;  // the GPU setup's own phases (PSX_TIMING)
bool g_have_setup_info = false;

void print_phases() {
    if (!getenv("PSX_TIMING")) return;
    const char* t0 = getenv("PSX_T0");
    const double spawn = t0 ? atof(t0) / 1e6 : g_ph.main;
    fprintf(stderr,
            "psx-timing {\"to_main_ms\": %.3f, \"args_ms\": %.3f, \"parse_ms\": %.3f, \"hip_runtime_ms\": %.3f, "
            "\"context_and_code_load_ms\": %.3f, \"wait_for_gpu_ms\": %.3f, \"gpu_setup_ms\": %.3f, "
            "\"sweep_ms\": %.3f, \"readback_ms\": %.3f, \"write_ms\": %.3f, \"teardown_ms\": %.3f, "
            "\"end_epoch_ms\": %.3f}\n",
            g_ph.main - spawn, g_ph.parse0 - g_ph.main, g_ph.parse1 - g_ph.parse0, g_ph.rt1 - g_ph.rt0, g_ph.warm1 - g_ph.rt1,
            g_ph.joined - g_ph.parse1, g_ph.setup1 - g_ph.joined, g_ph.sweep1 - g_ph.setup1,
            g_ph.accum1 - g_ph.sweep1, g_ph.write1 - g_ph.accum1, g_ph.end - g_ph.write1, g_ph.end);
    if (g_have_setup_info) {
        const psx_setup_info& i = g_setup_info;
        fprintf(stderr,
                "psx-setup {\"setup_ms\": %.3f, \"alloc_ms\": %.3f, \"studies_ms\": %.3f, \"tail_ms\": %.3f, "
                "\"upload_ms\": [%.3f, %.3f], \"psd_lu_ms\": [%.3f, %.3f], \"finish_ms\": [%.3f, %.3f]}\n",
                i.setup_ms, i.alloc_ms, i.studies_ms, i.tail_ms, i.study_upload_ms[0], i.study_upload_ms[1],
                i.study_psd_ms[0], i.study_psd_ms[1], i.study_finish_ms[0], i.study_finish_ms[1]);
    }
}

// postcal.cpp:1166-1236 (stdout only): per study, the SNPs ranked by
// exp(post - total) with util.h:23-27's by_number (|x| descending) through the
// same std::sort, then the walk to the -r credible mass printing "index pip" for
// ranked PIPs above the -a threshold.  Reproduces the reference's indexing as
// written: study s's ranks are read from items[0 .. M_s) (study 0's sorted
// range), and the printed pip is the unranked SNP's at start + index.
struct RankItem {
    double number;
    int index1, index2;
};
void print_credible_listing(const vector<double>& post, double total, const vector<int>& m, double input_rho,
                            double threshold) {
    const int N = (int)post.size();
    vector<RankItem> items;
    items.reserve(N);
    for (int i = 0; i < N; i++) items.push_back(RankItem{std::exp(post[i] - total), i, 0});
    printf("\n");
    vector<int> rank(N, 0);
    int start = 0, end = 0;
    for (int s = 0; s < 2; s++) {
        end += m[s];
        printf("start offset = %d\n", start);
        printf("end offset = %d\n", end);
        std::sort(items.begin() + start, items.begin() + end,
                  [](const RankItem& l, const RankItem& r) { return std::fabs(l.number) > std::fabs(r.number); });
        printf("sort complete %d\n", s);
        for (int i = 0; i < m[s]; i++) rank[start + i] = items[i].index1;
        start = end;
    }
    std::cout << "threshold is " << threshold << "\n";
    start = end = 0;
    for (int s = 0; s < 2; s++) {
        end += m[s];
        double r = 0;
        int index = 0;
        while (r < input_rho) {
            const double ranked = special_exp(post[rank[start + index]], total);
            r += ranked;
            if (ranked > threshold) {
                const double pip = special_exp(post[start + index], total);
                if (pip > 0.01) printf("%d %f\n", start + index, pip);
            }
            index++;
            if (index >= m[s]) break;
        }
        start = end;
    }
    printf("\n");
}

int die_engine(int rc) {
    std::cout << "engine error (" << rc << "): " << (g_multi ? psx_multi_last_error() : psx_last_error()) << std::endl;
    if (rc == PSX_ESINGULAR) {
        std::cout << "Error the matrix is singular and we fail to fix it (low rank lkl)." << std::endl;
        exit(0);  // postcal.cpp:291-294
    }
    if (rc == PSX_EORDER) {
        printf("This did not work as expected\n");
        exit(1);
    }
    exit(1);
}

}  // namespace

int main(int argc, char* argv[]) {
    g_ph.main = epoch_ms();
    int totalCausalSNP = 3;  // pipsort.cpp:69-77
    double gamma = 0.01, sharing_param = 0.75, rho = 0.95, tau_sqr = 0.52, sigma_g_squared = 5.2;
    double cutoff_threshold = 0;
    string ldFile = "", zFile = "", snpMapFile = "", outputFileName = "", sample_s = "", num_causal_s = "";
    string configsFile = "";
    int num_groups = 0, num_configs = 0, sss_flag = 0, oc = 0;
    while ((oc = getopt(argc, argv, "vhl:o:z:m:p:r:c:k:g:f:t:s:n:a:b:d:e:q:x")) != -1) {
        if (optarg == NULL || *optarg == '\0') {  // pipsort.cpp:92-95
            printf("optarg is NULL\n");
            exit(1);
        }
        switch (oc) {
            case 'l': ldFile = optarg; break;
            case 'o': outputFileName = optarg; break;
            case 'z': zFile = optarg; break;
            case 'm': snpMapFile = optarg; /* falls through, pipsort.cpp:128-131 */
            case 'n': sample_s = optarg; break;
            case 'b': configsFile = optarg; break;
            case 'd': num_configs = atoi(optarg); break;
            case 'e': num_groups = atoi(optarg); break;
            case 'p': sharing_param = atof(optarg); break;
            case 'r': rho = atof(optarg); break;
            case 'c': totalCausalSNP = atoi(optarg); break;
            case 'k': num_causal_s = optarg; break;
            case 'g': gamma = atof(optarg); break;
            case 'f': break;
            case 't': tau_sqr = atof(optarg); break;
            case 's': sigma_g_squared = atof(optarg); break;
            case 'q': sss_flag = std::stoi(optarg); break;
            case ':':
            case '?':
            case 'a': cutoff_threshold = atof(optarg); break;
            case 'x': printf("Hello world flag x\n"); break;
            default: break;
        }
    }
    if (ldFile == "" || zFile == "" || snpMapFile == "" || outputFileName == "" || sample_s == "") {
        std::cout << "Error: -l, -z, -o, and -n are required" << std::endl;
        exit(1);
    }
    if (configsFile != "") {
        if (num_configs <= 0) {
            std::cout << "Number of configs must be greater than 0" << std::endl;
            exit(1);
        }
        if (num_groups <= 0) std::cout << "Number of groups must be greater than 0" << std::endl;
    }
    vector<string> ldDir = read_dir(ldFile), zDir = read_dir(zFile);
    vector<int> sample_sizes = read_sigma(sample_s);
    if (ldDir.size() != zDir.size() || ldDir.size() != sample_sizes.size()) {
        std::cout << "Error: LD files, Z files, and sample sizes do not match in number" << std::endl;
        exit(1);
    }
    const int S = (int)ldDir.size();
    if (S != 2) {
        std::cout << "This prior does not work for more than 2 studies yet\n";
        exit(1);
    }
    auto t_setup0 = std::chrono::steady_clock::now();
    // Devices: PSX_DEVICE (default 0) runs the sweep on one GPU.  Several GPUs
    // in one process (psx_multi, the analogue of the reference's whole-node
    // OpenMP threads, postcal.cpp:747-769) are opt-in: PSX_DEVICES="0,1,.."
    // (entries may repeat), or PSX_DEVICES=auto, which takes one more visible
    // device per 5e11 configurations of an exhaustive sweep (each extra device
    // costs its own context and Model setup, ~0.1-0.2 s, while one MI355X
    // sweeps ~4.5e12 configurations/s; SSS walks and -b files stay on one).
    vector<int32_t> devices;
    bool defer_devices = false;
    const char* ds = getenv("PSX_DEVICES");
    if (ds && string(ds) == "auto") {
        devices.push_back(0);
        defer_devices = true;  // decided once the locus size is known
    } else if (ds) {
        std::stringstream ss(ds);
        string tok;
        while (std::getline(ss, tok, ','))
            if (!tok.empty()) devices.push_back(atoi(tok.c_str()));
    } else if (const char* d = getenv("PSX_DEVICE")) {
        devices.push_back(atoi(d));
    } else {
        devices.push_back(0);
    }
    if (devices.empty()) devices.push_back(0);
    // -q 1 with -c 7..10: the wide SSS walk (psx_run_sss_wide), which runs on one handle
    const bool sss_wide = sss_flag == 1 && totalCausalSNP > 6;
    if (sss_wide && ds) {
        fprintf(stderr, "PIPSORT: -q 1 -c %d runs on one device (%d); PSX_DEVICES is not used\n", totalCausalSNP,
                (int)devices[0]);
        devices.resize(1);
        defer_devices = false;
    }
    const int device = devices[0];
    g_multi = devices.size() > 1;
    // one locus per process: one stream (hardware queue) per device for the
    // whole run — each queue costs ~10-13 ms when the process exits
    // (PSX_SINGLE_QUEUE=0: the engine's own streams, for A/B)
    const char* sq = getenv("PSX_SINGLE_QUEUE");
    psx_single_queue(sq ? atoi(sq) : 1);
    // the HIP runtime / contexts come up on a second thread while the inputs
    // are parsed (errors, if any, surface again at psx_create*)
    // (SSS batches run the generic set kernel; the wide walk its own code object, loaded for -c > 6)
    const int warm_c = sss_flag == 1 && !sss_wide ? 0 : totalCausalSNP;
    const int warm_b = configsFile != "";
    std::thread warm([devices, warm_c, warm_b] {
        g_ph.rt0 = epoch_ms();
        int nd = 0;
        psx_device_count(&nd);  // the HIP runtime
        g_ph.rt1 = epoch_ms();
        vector<int32_t> seen;
        for (int32_t d : devices)
            if (std::find(seen.begin(), seen.end(), d) == seen.end()) {
                seen.push_back(d);
                psx_warmup_for(d, warm_c, warm_b);
            }
        g_ph.warm1 = epoch_ms();
    });
    auto quit = [&warm](int code) {  // input errors below exit as the reference does, after the warm-up
        warm.join();
        exit(code);
    };
    // ---- Model (model.h:86-264) ----
    g_ph.parse0 = epoch_ms();
    vector<vector<double>> sig(S), zs(S);
    vector<vector<string>> names(S);
    vector<int> m(S);
    for (int i = 0; i < S; i++) {
        vector<double> L;
        if (!import_data(ldDir[i], L)) quit(1);
        import_z(zDir[i], names[i], zs[i]);
        int M = (int)std::sqrt((double)L.size());  // model.h:98
        m[i] = M;
        if (M != (int)names[i].size()) {
            printf("ERROR: LD matrix is size %d x %d but zscores has %lu snps\n. Check LD file for nans.\n", M, M,
                   (unsigned long)names[i].size());
            quit(1);
        }
        printf("pushing back num snps %d for study %d\n", i, M);
        L.resize((size_t)M * M);
        sig[i] = std::move(L);
    }
    vector<string> all_snp_pos;
    vector<vector<int>> u2l(S);
    if (!import_snp_map(snpMapFile, S + 1, all_snp_pos, u2l)) quit(1);
    const int U = (int)all_snp_pos.size();
    for (int i = 0; i < S; i++) {  // model.h:134-144
        int cnt = 0;
        if ((int)u2l[i].size() != U) { printf("Invariant does not hold\n"); quit(1); }
        for (int u = 0; u < U; u++) cnt += u2l[i][u] >= 0;
        if (cnt != m[i]) { printf("Invariant does not hold\n"); quit(1); }
    }
    const int N = m[0] + m[1];
    if (defer_devices && configsFile == "" && sss_flag != 1) {
        // configurations of the exhaustive sweep: sum_k e_k(w_u), w_u = 2^{b_u} - 1
        vector<long double> ek(totalCausalSNP + 1, 0.0L);
        ek[0] = 1;
        for (int u = 0; u < U; u++) {
            const int b = (u2l[0][u] >= 0) + (u2l[1][u] >= 0);
            for (int k = totalCausalSNP; k >= 1; k--) ek[k] += ek[k - 1] * (long double)((1 << b) - 1);
        }
        long double configs = 0;
        for (long double v : ek) configs += v;
        int nd = 0;
        psx_device_count(&nd);
        const int want = (int)std::min<long double>((long double)std::max(nd, 1), 1.0L + configs / 5e11L);
        for (int i = 1; i < want; i++) devices.push_back(i);
        g_multi = devices.size() > 1;
    }
    vector<int32_t> u2l_flat(2 * U);
    for (int s = 0; s < 2; s++)
        for (int u = 0; u < U; u++) u2l_flat[s * U + u] = u2l[s][u];
    g_ph.parse1 = epoch_ms();
    warm.join();
    g_ph.joined = epoch_ms();
    psx_engine* eng = nullptr;
    psx_multi* multi = nullptr;
    int rc;
    const char* hs = getenv("PSX_HOST_SETUP");
    if (!(hs && atoi(hs))) {
        // Model setup on the GPU (model.h:171-264): PSD shift by device LU, then
        // Sigma~ = Sigma', y = z, ||S'||^2 = z^T Sigma'^-1 z when Sigma' is PD
        vector<double> ld, z;
        ld.reserve((size_t)m[0] * m[0] + (size_t)m[1] * m[1]);
        for (int i = 0; i < S; i++) {
            ld.insert(ld.end(), sig[i].begin(), sig[i].end());
            z.insert(z.end(), zs[i].begin(), zs[i].end());
        }
        psx_ld_problem q;
        q.n_studies = 2;
        q.m = m.data();
        q.ld = ld.data();
        q.z = z.data();
        q.n_union = U;
        q.union_to_local = u2l_flat.data();
        q.max_causal = totalCausalSNP;
        q.sample_sizes = sample_sizes.data();
        q.sharing_param = sharing_param;
        q.gamma = gamma;
        q.t_squared = tau_sqr;
        q.s_squared = sigma_g_squared;
        psx_setup_info info;
        if (g_multi)
            rc = psx_multi_create_from_ld(&q, devices.data(), (int32_t)devices.size(), &multi, &info);
        else
            rc = psx_create_from_ld(&q, device, &eng, &info);  // model.h:171-265
        if (rc == 0) {
            g_setup_info = info;
            g_have_setup_info = true;
        }
        if (rc == 0)
            for (int i = 0; i < S; i++)
                std::cout << "study " << i << ": psd shift " << info.psd_added[i] << " ("
                          << info.psd_iterations[i] << " LU), "
                          << (info.eigen_route[i] ? "eigen route" : "positive definite, no eigen") << std::endl;
    } else {
        // host restatement of the reference setup (PSX_HOST_SETUP=1)
        vector<double> B, sp(N);
        size_t boff = 0;
        int off = 0;
        B.resize((size_t)m[0] * m[0] + (size_t)m[1] * m[1]);
        for (int i = 0; i < S; i++) {
            auto b0 = std::chrono::steady_clock::now();
            double add = 0;
            psx_psd_shift(sig[i].data(), m[i], &add);  // model.h:194
            auto b1 = std::chrono::steady_clock::now();
            std::cout << "Time to make psd = "
                      << std::chrono::duration_cast<std::chrono::microseconds>(b1 - b0).count() << "[µs]" << std::endl;
            psx_lowrank_study(sig[i].data(), zs[i].data(), m[i], B.data() + boff, sp.data() + off);  // model.h:213-259
            auto b2 = std::chrono::steady_clock::now();
            std::cout << "Time for eigen decomp = "
                      << std::chrono::duration_cast<std::chrono::microseconds>(b2 - b1).count() << "[µs]" << std::endl;
            boff += (size_t)m[i] * m[i];
            off += m[i];
        }
        psx_problem prob;
        prob.n_studies = 2;
        prob.m = m.data();
        prob.B = B.data();
        prob.s_prime = sp.data();
        prob.n_union = U;
        prob.union_to_local = u2l_flat.data();
        prob.max_causal = totalCausalSNP;
        prob.sample_sizes = sample_sizes.data();
        prob.sharing_param = sharing_param;
        prob.gamma = gamma;
        prob.t_squared = tau_sqr;
        prob.s_squared = sigma_g_squared;
        rc = g_multi ? psx_multi_create(&prob, devices.data(), (int32_t)devices.size(), &multi)
                     : psx_create(&prob, device, &eng);  // model.h:265
    }
    if (rc) die_engine(rc);
    g_ph.setup1 = epoch_ms();
    auto t_setup1 = std::chrono::steady_clock::now();
    std::cout << "Time for setup = " << std::chrono::duration_cast<std::chrono::microseconds>(t_setup1 - t_setup0).count()
              << "[µs]" << std::endl;
    // ---- findOptimalSetGreedy (postcal.cpp:1128-1244) ----
    std::cout << "Max Causal = " << totalCausalSNP << std::endl;
    std::cout << "Union Snp Count = " << U << std::endl;
    auto t0 = std::chrono::steady_clock::now();
    if (configsFile != "") {
        int fd = open(configsFile.c_str(), O_RDONLY);  // util.cpp:26-49
        if (fd < 0) {
            printf("Could not open %s\n", configsFile.c_str());
            printf("mmap did not succeed\n");
            exit(1);
        }
        struct stat st;
        fstat(fd, &st);
        size_t sz = (size_t)st.st_size;
        if ((size_t)num_configs * num_groups * sizeof(int16_t) != sz) {  // postcal.cpp:434-437
            printf("config file is not the expected size\n");
            exit(1);
        }
        void* p = sz ? mmap(nullptr, sz, PROT_READ, MAP_SHARED, fd, 0) : nullptr;
        close(fd);
        rc = g_multi ? psx_multi_run_configs(multi, (const int16_t*)p, num_configs, num_groups)
                     : psx_run_configs(eng, (const int16_t*)p, num_configs, num_groups);
        if (p) munmap(p, sz);
    } else if (sss_flag == 1) {
        int32_t iters = 0;
        rc = sss_wide ? psx_run_sss_wide(eng, &iters)
             : g_multi ? psx_multi_run_sss(multi, &iters) : psx_run_sss(eng, &iters);
        printf("sss iterations = %d\n", iters);
    } else {
        rc = g_multi ? psx_multi_run_exhaustive(multi) : psx_run_exhaustive(eng);
    }
    if (rc) die_engine(rc);
    g_ph.sweep1 = epoch_ms();
    auto t1 = std::chrono::steady_clock::now();
    std::cout << "Time to eval all= " << std::chrono::duration_cast<std::chrono::microseconds>(t1 - t0).count()
              << "[µs]" << std::endl;
    vector<double> post(N), noc(2), shared(U), sll(U), nsll(U);
    psx_accum acc;
    acc.post = post.data();
    acc.no_causal = noc.data();
    acc.shared = shared.data();
    acc.shared_ll = sll.data();
    acc.notshared_ll = nsll.data();
    if ((rc = g_multi ? psx_multi_get_accum(multi, &acc) : psx_get_accum(eng, &acc))) die_engine(rc);
    g_ph.accum1 = epoch_ms();
    psx_timing tm;
    if (g_multi)
        psx_multi_get_timing(multi, &tm);
    else
        psx_get_timing(eng, &tm);
    printf("num total configs = %llu\n", (unsigned long long)acc.n_configs);
    if (g_multi) printf("devices = %d (one shard each, folded on device %d)\n", (int)devices.size(), device);
    printf("sweep device time = %.3f ms (kernel %.3f ms, merge %.3f ms)\n", tm.sweep_ms, tm.kernel_ms, tm.merge_ms);
    const double total = acc.total;
    {
        std::ofstream lf((outputFileName + "_log.txt").c_str(), std::ios::out | std::ios::app);  // util.cpp:183-187
        lf << std::exp(total) << std::endl;
    }
    // postcal.cpp:1145-1148: addlogSpace (postcal.h:102-112) over postValues in index order
    double total_post = 0;
    for (int i = 0; i < N; i++) {
        const double a = total_post, b = post[i];
        if (a == 0) { total_post = b; continue; }
        if (b == 0) continue;
        const double base = std::max(a, b);
        total_post = (base - std::min(a, b) > 700) ? base : base + std::log(1 + std::exp(std::min(a, b) - base));
    }
    printf("\nTotal Likelihood = %e SNP=%d \n", total_post, N);
    printf("total post as total likelihood log = %f\n", total);
    for (int i = 0; i < 2; i++) {
        printf("no causal just value %f\n", noc[i]);
        printf("Prob of no causal for study %d is %f\n", i, std::exp(noc[i] - total));
    }
    vector<char> causalSet(N, '0');
    for (int i = 0; i < N; i++)
        if (special_exp(post[i], total) > 0.05) causalSet[i] = '1';  // postcal.cpp:1158-1164
    print_credible_listing(post, total, m, rho, cutoff_threshold);
    // ---- finishUp (model.h:282-310) + printPost2File (postcal.h:288-336) ----
    int so = 0;
    for (int s = 0; s < 2; s++) {
        std::ofstream f((outputFileName + "_study" + std::to_string(s) + "_set.txt").c_str());
        for (int j = 0; j < m[s]; j++)
            if (causalSet[so + j] == '1') f << names[s][j] << std::endl;
        so += m[s];
    }
    so = 0;
    for (int s = 0; s < 2; s++) {
        std::ofstream f((outputFileName + "_study" + std::to_string(s) + "_post.txt").c_str());
        f << "SNP_ID\tProb_in_pCausalSet" << std::endl;
        for (int j = 0; j < m[s]; j++) f << names[s][j] << "\t" << special_exp(post[so + j], total) << std::endl;
        so += m[s];
    }
    {
        std::ofstream f((outputFileName + "_nocausal.txt").c_str());
        for (int s = 0; s < 2; s++) f << special_exp(noc[s], total) << std::endl;
    }
    {
        std::ofstream f((outputFileName + "_shared_pips.txt").c_str());
        f << "SNP_ID\tshared_pip\tshared_ll\tnotshared_ll" << std::endl;
        for (int u = 0; u < U; u++)
            f << all_snp_pos[u] << "\t" << special_exp(shared[u], total) << "\t" << sll[u] << "\t" << nsll[u]
              << std::endl;
    }
    std::cout.flush();
    g_ph.write1 = epoch_ms();
    if (g_multi)
        psx_multi_destroy(multi);
    else
        psx_destroy(eng);
    (void)num_causal_s;
    g_ph.end = epoch_ms();
    print_phases();
    // Every output is written and the engine destroyed (its device work done,
    // its memory freed).  Returning from main would now run the HIP runtime's
    // static teardown, ~0.1 s on MI355X (bench example_wall_phases.exit_ms) — a
    // third of the whole tests/example run; the kernel reclaims the process's
    // device resources at exit either way, so leave directly, exit status 0.
    fflush(nullptr);
    _exit(0);
}
