// main.cpp -- drop-in for `./BayesianNetwork -a 0|2|4|5|6|7|8|10|12|13 ...` (src/main.cpp:17-201, src/Parameter.cpp:6-107):
// same flags, defaults and "../dataset/" path prefix; -a 0 (PC-stable), -a 2 (junction tree), -a 4
// (probabilistic logic sampling), -a 5 (likelihood weighting; -q samples per case, the reference's
// default 10000), -a 6 (EPIS-BN; -q samples per case after -d iterations of LBP) and -a 7 (loopy belief
// propagation; -d propagation length, the reference's default 2), -a 10 (AIS-BN) and -a 8 (SIS; both: -q
// samples per case, -m maximum updates, default 10, -l updating interval, default 2,500) run on the GPU.
// -a 9 ("SISv1") stays refused: the reference defines it nowhere.  Extra flags: --device N, --gpus G (devices N .. N + G - 1, RCCL: MultiGpu.h),
// --depth D (PC-stable max depth, reference default 1000), --seed N (sampling seed, 0), --tol T and
// --damping L (LBP: stop once an iteration's residual is <= T, default 0; damping in [0, 1), default 0),
// --eps E (the cutoff of EPIS-BN, AIS-BN and SIS in [0, 1); default: by state count).
// -a 12 is this build's own: the most probable explanation (MPE) of every case of the testing set.  The
// reference's -a stops at 11 and it has no MPE, so there is no reference output to match: the header
// block is in the house style, the result lines are the case count, the mean log P(x*, e) and the kernel
// time; --out FILE writes the assignments as LIBSVM rows (label = the value of variable 0).
// -a 13 is this build's own as well: expectation-maximisation (EM) of the CPTs of -f0's structure, from
// -f0's parameters, on the rows of -f3 (LIBSVM; a variable a row does not list is missing): -d iterations,
// --tol the relative stopping tolerance, pseudo-count 1; one line per iteration with the log-likelihood and
// Q; --out FILE writes the learned CPTs as text, one line per node and parent configuration.
// -a 14, this build's own too: score-based structure learning, greedy hill climbing over arc additions,
// deletions and reversals from the empty graph on -f2's CSV (--score bic|aic|loglik|bde|k2, default bic; bic-g|aic-g|loglik-g|bge: -f2 is a CSV of reals, the Gaussian scores, -a 14 only;
// --iss X: the equivalent sample size of bde, default 1, refused beside any other score; --max-parents K);
// prints the arc count, the score and the iterations, and with -f1 given the SHD against
// that network through -a 0's comparison; --out FILE writes the DAG, one line per node: node, number of
// parents, parents ascending.  --device -1 runs the host twin (same result, bit for bit).
// -a 17, this build's own: exact score-optimal structure learning on -a 14's inputs, flags and output shape
// (arcs, score, SHD against -f1, --out): the globally best DAG by dynamic programming over variable subsets;
// a dataset of more than 26 variables is refused with the limit's message.
// -a 18, this build's own: exact arc posteriors on -a 17's inputs and flags (--prior uniform|indegree, default
// uniform): P(u -> v | data) for every arc by Bayesian model averaging on the same subset lattices; prints logZ
// and the arcs with posterior >= 0.5, one per line; --out writes the full matrix, row u = the arcs out of u;
// -a 20, this build's own: the same arc posteriors for up to 64 variables by MCMC over node orders, on -a 18's
// inputs and flags (--max-parents defaults to 3 here) plus -q chains (default 64), -m burn-in steps (2000), -l samples
// per chain (200), --thin steps between samples (20), --seed; prints the arcs with posterior >= 0.5, the mean
// acceptance rate and the largest between-chain standard error of an arc; --out writes the full matrix as -a 18.
// -a 19, this build's own: PC-stable on continuous data: -f2 is a CSV of reals (a header line, then rows of numbers);
// Fisher-z tests of the partial correlation at alpha 0.05, --depth as -a 0; prints -a 0's lines (tests per level,
// remaining edges, SHD against -f1 when given); --out FILE writes the learned PDAG, one edge per line: from, to, 1
// for an arc; min, max, 0 for an undirected edge.
// -a 15, this build's own: exact posterior sampling on -a 12's inputs: -q draws per case from P(x | e) under
// --seed; prints the case count, the average log P(e) and the kernel time; --out FILE writes the drawn rows
// as LIBSVM, the -q rows of a case one after the other (label = the value of variable 0).
// -a 16, this build's own: Gibbs sampling on -a 10's inputs and flags: -q chains per case, -m burn-in sweeps,
// -l counted sweeps (their defaults are -a 10's: 10000, 10, 2500), --seed; prints -a 10's result lines.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

#include "JunctionTree.h"
#include "PCStable.h"
#include "fastbn.h"

// What the score-based learners (-a 14, 17, 18, 20) share ahead of their entries: the discrete sample set and
// --score / --iss as the entries take them.

struct DiscreteSet {
    int n = 0;
    int64_t ns = 0;
    std::vector<int32_t> dims;
    std::vector<uint8_t> cols;
};

// -f2's CSV into its columns; false: fbn_last_error() says why
static bool LoadDiscreteSet(const std::string &path, DiscreteSet *d) {
    fbn_dataset *ds = nullptr;
    if (fbn_dataset_load_csv(path.c_str(), &ds)) return false;
    fbn_dataset_shape(ds, &d->n, &d->ns);
    d->dims.resize((size_t)d->n);
    d->cols.resize((size_t)d->n * (size_t)d->ns);
    fbn_dataset_dims(ds, d->dims.data());
    fbn_dataset_columns(ds, d->cols.data());
    fbn_dataset_destroy(ds);
    return true;
}

static bool IsGaussScore(const std::string &s) { return s == "bic-g" || s == "aic-g" || s == "loglik-g" || s == "bge"; }

// the refusal of a learner that takes discrete data only
static int RefuseGaussScore(const std::string &score_name, int algorithm) {
    fprintf(stderr, "Error: --score %s scores continuous data, which -a %d does not learn from (hill climbing, -a 14, does)\n",
            score_name.c_str(), algorithm);
    return 1;
}

// A Bayesian Dirichlet score (BDeu with --iss, K2) has no penalty term and goes through the _bd entries; every
// other name is a penalty per free parameter.  0, or 1 with the refusal printed.
struct LearnerScore {
    bool is_bd = false;
    fbn_bd_score bd{};
    double penalty = 0.0;
};
static int ParseLearnerScore(const std::string &score_name, bool iss_given, double iss, int64_t ns, LearnerScore *s) {
    s->is_bd = score_name == "bde" || score_name == "k2";
    if (iss_given && score_name != "bde") {
        fprintf(stderr, "Error: --iss is the equivalent sample size of --score bde; the score is %s\n", score_name.c_str());
        return 1;
    }
    s->bd = fbn_bd_score{score_name == "k2" ? FBN_SCORE_K2 : FBN_SCORE_BDE, 0, iss};
    if (!s->is_bd && fbn_hc_penalty(score_name.c_str(), ns, &s->penalty)) {
        fprintf(stderr, "Error: %s\n", fbn_last_error());
        return 1;
    }
    return 0;
}

int main(int argc, char **argv) {
    int algorithm = 2, num_threads = 1, group_size = 1, device = 0, depth = 1000, gpus = 1, propagation_length = 2;
    double tol = 0.0, damping = 0.0, eps = -1.0;
    long long num_samples = 10000, max_updating = 10, updating_interval = 2500;  // src/Parameter.cpp:14-15
    unsigned long long seed = 0;
    std::string out_file, score_name = "bic", prior_name = "uniform";
    int max_parents = -1;
    double iss = 1.0;
    bool ref_given = false, iss_given = false, q_given = false, m_given = false, l_given = false;
    long long thin = 20;
    std::string net_file = "alarm/alarm.xml", ref_net_file = "alarm/alarm.bif",
                train_set_file = "alarm/alarm_s5000.txt", test_set_file = "alarm/testing_alarm_1k_p20",
                pt_file = "alarm/alarm_1k_pt", prefix = "../dataset/";
    int i;
    for (i = 1; i < argc && argv[i][0] == '-'; i++) {
        std::string a = argv[i];
        if (a == "--device" && i + 1 < argc) { device = atoi(argv[++i]); continue; }
        if (a == "--gpus" && i + 1 < argc) { gpus = atoi(argv[++i]); continue; }
        if (a == "--depth" && i + 1 < argc) { depth = atoi(argv[++i]); continue; }
        if (a == "--prefix" && i + 1 < argc) { prefix = argv[++i]; continue; }
        if (a == "--seed" && i + 1 < argc) { seed = strtoull(argv[++i], nullptr, 10); continue; }
        if (a == "--tol" && i + 1 < argc) { tol = atof(argv[++i]); continue; }
        if (a == "--damping" && i + 1 < argc) { damping = atof(argv[++i]); continue; }
        if (a == "--eps" && i + 1 < argc) { eps = atof(argv[++i]); continue; }
        if (a == "--out" && i + 1 < argc) { out_file = argv[++i]; continue; }
        if (a == "--score" && i + 1 < argc) { score_name = argv[++i]; continue; }
        if (a == "--iss" && i + 1 < argc) { iss = atof(argv[++i]); iss_given = true; continue; }
        if (a == "--max-parents" && i + 1 < argc) { max_parents = atoi(argv[++i]); continue; }
        if (a == "--prior" && i + 1 < argc) { prior_name = argv[++i]; continue; }
        if (a == "--thin" && i + 1 < argc) { thin = atoll(argv[++i]); continue; }
        switch (argv[i][1]) {
        case 'h':
            std::cout << "Usage: ./BayesianNetwork [-a 0|2|4|5|6|7|8|10|12|13|14|15|16|17|18|19|20] [-t threads] [-g group] [-q samples] [-d length] [-m updates] "
                         "[-l interval] [-f0 net] "
                         "[-f1 refnet] [-f2 train] [-f3 test] [-f4 pt] [--device N] [--gpus G] [--depth D] [--seed N] "
                         "[--tol T] [--damping L] [--eps E] [--score bic|aic|loglik|bde|k2|bic-g|aic-g|loglik-g|bge] [--iss X] [--max-parents K] [--prior uniform|indegree] [--thin T] "
                         "[--out FILE] [--prefix DIR]"
                      << std::endl;
            return 0;
        case 'a': algorithm = atoi(argv[++i]); break;
        case 't': num_threads = atoi(argv[++i]); break;
        case 'g': group_size = atoi(argv[++i]); break;
        case 'q': num_samples = atoll(argv[++i]); q_given = true; break;
        case 'd': propagation_length = atoi(argv[++i]); break;  // src/Parameter.cpp:40
        case 'm': max_updating = atoll(argv[++i]); m_given = true; break;      // src/Parameter.cpp:38
        case 'l': updating_interval = atoll(argv[++i]); l_given = true; break;  // src/Parameter.cpp:39
        case 'f':
            switch (argv[i][2]) {
            case '0': net_file = argv[++i]; break;
            case '1': ref_net_file = argv[++i]; ref_given = true; break;
            case '2': train_set_file = argv[++i]; break;
            case '3': test_set_file = argv[++i]; break;
            case '4': pt_file = argv[++i]; break;
            }
            break;
        default:
            printf("\n Unrecognized option %s!\n", argv[i]);
            return 0;
        }
    }
    net_file = prefix + net_file;
    ref_net_file = prefix + ref_net_file;
    train_set_file = prefix + train_set_file;
    test_set_file = prefix + test_set_file;
    pt_file = prefix + pt_file;

    if (algorithm == 0) {
        std::cout << "===============================" << std::endl
                  << "Algorithm: PC-stable for structure learning, #threads = " << num_threads << std::endl
                  << "group size = " << group_size << std::endl
                  << "\treference BN: " << ref_net_file << std::endl
                  << "\tsample set: " << train_set_file << std::endl
                  << "===============================" << std::endl;
        fbn_dataset *ds = nullptr;
        if (fbn_dataset_load_csv(train_set_file.c_str(), &ds)) {
            fprintf(stderr, "Error: %s\n", fbn_last_error());
            return 1;
        }
        PCStable pc(0.05, depth, device, gpus);
        pc.StructLearnCompData(ds, group_size, num_threads, false, false);
        fbn_dataset_destroy(ds);
        std::cout << "SHD = " << pc.GetSHD(ref_net_file) << std::endl;
    } else if (algorithm == 2) {
        std::cout << "===============================" << std::endl
                  << "Algorithm: junction tree (JT) for exact inference, #threads = " << num_threads << std::endl
                  << "\tBN: " << net_file << std::endl
                  << "\ttesting set: " << test_set_file << std::endl
                  << "\treference potential table: " << pt_file << std::endl
                  << "===============================" << std::endl;
        fbn_network *net = nullptr;
        if (fbn_network_load_xmlbif(net_file.c_str(), &net)) {
            fprintf(stderr, "Error: %s\n", fbn_last_error());
            return 1;
        }
        int n = 0;
        fbn_network_num_nodes(net, &n);
        TestSet tester;
        if (tester.Load(test_set_file, n)) {
            fprintf(stderr, "Error: %s\n", fbn_last_error());
            return 1;
        }
        double accuracy;
        {
            JunctionTree jt(net, &tester, device, gpus);
            accuracy = jt.EvaluateAccuracy(pt_file, num_threads);
        }
        std::cout << "accuracy = " << accuracy << std::endl;
        fbn_network_destroy(net);
    } else if (algorithm == 4 || algorithm == 5) {
        // the reference's PLS / LW stubs (src/main.cpp:97-121): its header lines, then -a 2's result lines
        std::cout << "===============================" << std::endl
                  << (algorithm == 4 ? "Algorithm: probabilistic logic sampling (PLS) for approximate inference, #threads = "
                                     : "Algorithm: likelihood weighting (LW) for approximate inference, #threads = ")
                  << num_threads << std::endl
                  << "#samples = " << num_samples << std::endl
                  << "\tBN: " << net_file << std::endl
                  << "\ttesting set: " << test_set_file << std::endl
                  << "\treference potential table: " << pt_file << std::endl
                  << "===============================" << std::endl;
        auto die = [] {
            fprintf(stderr, "Error: %s\n", fbn_last_error());
            return 1;
        };
        fbn_network *net = nullptr;
        if (fbn_network_load_xmlbif(net_file.c_str(), &net)) return die();
        int n = 0;
        fbn_network_num_nodes(net, &n);
        TestSet tester;
        if (tester.Load(test_set_file, n)) return die();
        const int64_t nc = tester.num_instances();
        std::vector<int32_t> dims(n);
        fbn_network_dims(net, dims.data());
        int sum_dom = 0;
        for (int d : dims) sum_dom += d;
        std::vector<double> golden = LoadGroundTruth(pt_file, dims, nc);
        std::cout << "==================================================" << '\n'
                  << "Begin testing the trained network." << std::endl;
        fbn_sampler *smp = nullptr;
        if (fbn_sampler_create(net, device, &smp)) return die();
        std::vector<int32_t> predictions((size_t)nc);
        std::vector<double> marginals((size_t)nc * sum_dom);
        if (fbn_lw_run(smp, algorithm == 4 ? 1 : 0, tester.evidence.data(), nc, num_samples, seed, 0, predictions.data(),
                       marginals.data(), nullptr))
            return die();
        float kms = 0.f;
        const bool timed = fbn_sampler_last_kernel_ms(smp, &kms) == 0;  // not on the host path (--device -1)
        double mse = 0, hd = 0;
        if (fbn_score_marginals(net, marginals.data(), golden.data(), nc, &mse, &hd)) return die();
        int64_t correct = 0;
        for (int64_t c = 0; c < nc; ++c) correct += predictions[c] == tester.ground_truths[c];
        std::cout << "average MSE = " << mse / nc << std::endl;
        std::cout << "average HD = " << hd / nc << std::endl;
        std::cout << "==================================================" << std::endl;
        if (timed)
            std::cout << (algorithm == 4 ? "pls: " : "lw: ") << "device kernel " << kms * 1e-3 << " s, "
                      << (double)nc * (double)num_samples / (kms * 1e-3) << " samples/s" << std::endl;
        std::cout << "accuracy = " << correct / (double)nc << std::endl;
        fbn_sampler_destroy(smp);
        fbn_network_destroy(net);
    } else if (algorithm == 6) {
        // the reference's EPIS-BN stub (src/main.cpp:123-134): its header lines, then -a 2's result lines
        std::cout << "===============================" << std::endl
                  << "Algorithm: EPIS-BN for approximate inference, #threads = " << num_threads << std::endl
                  << "#samples = " << num_samples << ", propagation length = " << propagation_length << std::endl
                  << "\tBN: " << net_file << std::endl
                  << "\ttesting set: " << test_set_file << std::endl
                  << "\treference potential table: " << pt_file << std::endl
                  << "===============================" << std::endl;
        auto die = [] {
            fprintf(stderr, "Error: %s\n", fbn_last_error());
            return 1;
        };
        fbn_network *net = nullptr;
        if (fbn_network_load_xmlbif(net_file.c_str(), &net)) return die();
        int n = 0;
        fbn_network_num_nodes(net, &n);
        TestSet tester;
        if (tester.Load(test_set_file, n)) return die();
        const int64_t nc = tester.num_instances();
        std::vector<int32_t> dims(n);
        fbn_network_dims(net, dims.data());
        int sum_dom = 0;
        for (int d : dims) sum_dom += d;
        std::vector<double> golden = LoadGroundTruth(pt_file, dims, nc);
        std::cout << "==================================================" << '\n'
                  << "Begin testing the trained network." << std::endl;
        fbn_epis *ep = nullptr;
        if (fbn_epis_create(net, device, &ep)) return die();
        std::vector<int32_t> predictions((size_t)nc);
        std::vector<double> marginals((size_t)nc * sum_dom), stats((size_t)nc * 4);
        if (fbn_epis_run(ep, tester.evidence.data(), nc, num_samples, seed, 0, propagation_length, tol, damping, eps,
                         predictions.data(), marginals.data(), stats.data()))
            return die();
        float lms = 0.f, sms = 0.f;
        const bool timed = fbn_epis_last_kernel_ms(ep, &lms, &sms) == 0;  // not on the host path (--device -1)
        double mse = 0, hd = 0, ess = 0;
        if (fbn_score_marginals(net, marginals.data(), golden.data(), nc, &mse, &hd)) return die();
        int64_t correct = 0;
        for (int64_t c = 0; c < nc; ++c) correct += predictions[c] == tester.ground_truths[c], ess += stats[4 * c + 1];
        std::cout << "average MSE = " << mse / nc << std::endl;
        std::cout << "average HD = " << hd / nc << std::endl;
        std::cout << "average ESS = " << ess / nc << std::endl;
        std::cout << "==================================================" << std::endl;
        if (timed)
            std::cout << "epis: device kernels lbp " << lms * 1e-3 << " s, sampling " << sms * 1e-3 << " s, "
                      << (double)nc * (double)num_samples / (sms * 1e-3) << " samples/s" << std::endl;
        std::cout << "accuracy = " << correct / (double)nc << std::endl;
        fbn_epis_destroy(ep);
        fbn_network_destroy(net);
    } else if (algorithm == 7) {
        // the reference's LBP stub (src/main.cpp:136-147): its header lines, then -a 2's result lines
        std::cout << "===============================" << std::endl
                  << "Algorithm: loopy belief propagation (LBP) for approximate inference, #threads = " << num_threads
                  << std::endl
                  << ", propagation length = " << propagation_length << std::endl
                  << "\tBN: " << net_file << std::endl
                  << "\ttesting set: " << test_set_file << std::endl
                  << "\treference potential table: " << pt_file << std::endl
                  << "===============================" << std::endl;
        auto die = [] {
            fprintf(stderr, "Error: %s\n", fbn_last_error());
            return 1;
        };
        fbn_network *net = nullptr;
        if (fbn_network_load_xmlbif(net_file.c_str(), &net)) return die();
        int n = 0;
        fbn_network_num_nodes(net, &n);
        TestSet tester;
        if (tester.Load(test_set_file, n)) return die();
        const int64_t nc = tester.num_instances();
        std::vector<int32_t> dims(n);
        fbn_network_dims(net, dims.data());
        int sum_dom = 0;
        for (int d : dims) sum_dom += d;
        std::vector<double> golden = LoadGroundTruth(pt_file, dims, nc);
        std::cout << "==================================================" << '\n'
                  << "Begin testing the trained network." << std::endl;
        fbn_lbp *lbp = nullptr;
        if (fbn_lbp_create(net, device, &lbp)) return die();
        std::vector<int32_t> predictions((size_t)nc);
        std::vector<double> marginals((size_t)nc * sum_dom), stats((size_t)nc * 2);
        if (fbn_lbp_run(lbp, tester.evidence.data(), nc, propagation_length, tol, damping, predictions.data(),
                        marginals.data(), stats.data()))
            return die();
        float kms = 0.f;
        const bool timed = fbn_lbp_last_kernel_ms(lbp, &kms) == 0;  // not on the host path (--device -1)
        double mse = 0, hd = 0, iters = 0;
        if (fbn_score_marginals(net, marginals.data(), golden.data(), nc, &mse, &hd)) return die();
        int64_t correct = 0;
        for (int64_t c = 0; c < nc; ++c) correct += predictions[c] == tester.ground_truths[c], iters += stats[2 * c];
        std::cout << "average MSE = " << mse / nc << std::endl;
        std::cout << "average HD = " << hd / nc << std::endl;
        std::cout << "==================================================" << std::endl;
        if (timed)
            std::cout << "lbp: device kernel " << kms * 1e-3 << " s, " << iters / (kms * 1e-3) << " case-iterations/s"
                      << std::endl;
        std::cout << "accuracy = " << correct / (double)nc << std::endl;
        fbn_lbp_destroy(lbp);
        fbn_network_destroy(net);
    } else if (algorithm == 8 || algorithm == 10) {
        // the reference's SIS / AIS-BN stubs (src/main.cpp:149-160, :175-186): its header lines, then -a 2's result lines
        std::cout << "===============================" << std::endl
                  << (algorithm == 8 ? "Algorithm: self importance sampling (SIS) for approximate inference, #threads = "
                                     : "Algorithm: AIS-BN for approximate inference, #threads = ")
                  << num_threads << std::endl
                  << "#samples = " << num_samples << "updating interval = " << updating_interval
                  << "maximum updating times = " << max_updating << std::endl
                  << "\tBN: " << net_file << std::endl
                  << "\ttesting set: " << test_set_file << std::endl
                  << "\treference potential table: " << pt_file << std::endl
                  << "===============================" << std::endl;
        auto die = [] {
            fprintf(stderr, "Error: %s\n", fbn_last_error());
            return 1;
        };
        const int method = algorithm == 8 ? 1 : 0;
        fbn_network *net = nullptr;
        if (fbn_network_load_xmlbif(net_file.c_str(), &net)) return die();
        int n = 0;
        fbn_network_num_nodes(net, &n);
        TestSet tester;
        if (tester.Load(test_set_file, n)) return die();
        const int64_t nc = tester.num_instances();
        std::vector<int32_t> dims(n);
        fbn_network_dims(net, dims.data());
        int sum_dom = 0;
        for (int d : dims) sum_dom += d;
        std::vector<double> golden = LoadGroundTruth(pt_file, dims, nc);
        std::cout << "==================================================" << '\n'
                  << "Begin testing the trained network." << std::endl;
        fbn_ais *ais = nullptr;
        if (fbn_ais_create(net, device, &ais)) return die();
        std::vector<int32_t> predictions((size_t)nc);
        std::vector<double> marginals((size_t)nc * sum_dom), stats((size_t)nc * 4);
        if (fbn_ais_run(ais, method, tester.evidence.data(), nc, num_samples, max_updating, updating_interval, seed, 0, eps,
                        predictions.data(), marginals.data(), stats.data()))
            return die();
        float kms = 0.f;
        const bool timed = fbn_ais_last_kernel_ms(ais, &kms) == 0;  // not on the host path (--device -1)
        double mse = 0, hd = 0, ess = 0;
        if (fbn_score_marginals(net, marginals.data(), golden.data(), nc, &mse, &hd)) return die();
        int64_t correct = 0;
        for (int64_t c = 0; c < nc; ++c) correct += predictions[c] == tester.ground_truths[c], ess += stats[4 * c + 1];
        const double draws = method == 0 ? (double)max_updating * (double)updating_interval + (double)num_samples
                                         : (double)num_samples;
        std::cout << "average MSE = " << mse / nc << std::endl;
        std::cout << "average HD = " << hd / nc << std::endl;
        std::cout << "average ESS = " << ess / nc << std::endl;
        std::cout << "==================================================" << std::endl;
        if (timed)
            std::cout << (method == 0 ? "ais-bn: " : "sis: ") << "device kernel " << kms * 1e-3 << " s, "
                      << (double)nc * draws / (kms * 1e-3) << " samples/s" << std::endl;
        std::cout << "accuracy = " << correct / (double)nc << std::endl;
        fbn_ais_destroy(ais);
        fbn_network_destroy(net);
    } else if (algorithm == 12) {
        // most probable explanation: no counterpart in the reference (its -a ends at 11)
        std::cout << "===============================" << std::endl
                  << "Algorithm: most probable explanation (MPE) by max-product junction tree, #threads = " << num_threads
                  << std::endl
                  << "\tBN: " << net_file << std::endl
                  << "\ttesting set: " << test_set_file << std::endl
                  << "===============================" << std::endl;
        auto die = [] {
            fprintf(stderr, "Error: %s\n", fbn_last_error());
            return 1;
        };
        fbn_network *net = nullptr;
        if (fbn_network_load_xmlbif(net_file.c_str(), &net)) return die();
        int n = 0;
        fbn_network_num_nodes(net, &n);
        TestSet tester;
        if (tester.Load(test_set_file, n)) return die();
        const int64_t nc = tester.num_instances();
        fbn_mpe *mpe = nullptr;
        if (fbn_mpe_create(net, device, &mpe)) return die();
        std::vector<int8_t> assignment((size_t)nc * n);
        std::vector<double> value((size_t)nc * 2);
        if (fbn_mpe_run(mpe, tester.evidence.data(), nc, assignment.data(), value.data())) return die();
        float kms = 0.f;
        const bool timed = fbn_mpe_last_kernel_ms(mpe, &kms) == 0;  // not on the host path (--device -1)
        double sum = 0;
        for (int64_t c = 0; c < nc; ++c) sum += log(value[2 * c]) + value[2 * c + 1] * log(2.0);
        std::cout << "cases = " << nc << std::endl;
        char buf[64];
        snprintf(buf, sizeof buf, "%.12g", nc ? sum / nc : 0.0);
        std::cout << "mean log P(x*, e) = " << buf << std::endl;
        if (timed)
            std::cout << "mpe: device kernel " << kms * 1e-3 << " s, " << nc / (kms * 1e-3) << " cases/s" << std::endl;
        if (!out_file.empty()) {
            std::vector<int32_t> labels((size_t)nc);
            for (int64_t c = 0; c < nc; ++c) labels[c] = assignment[(size_t)c * n];
            if (fbn_write_libsvm(out_file.c_str(), assignment.data(), nc, n, labels.data())) return die();
            std::cout << "assignments written to " << out_file << std::endl;
        }
        fbn_mpe_destroy(mpe);
        fbn_network_destroy(net);
    } else if (algorithm == 13) {
        // expectation-maximisation: no counterpart in the reference (its parameter learning assumes complete data)
        std::cout << "===============================" << std::endl
                  << "Algorithm: expectation-maximisation (EM) for parameter learning from incomplete data, #threads = "
                  << num_threads << std::endl
                  << "iterations = " << propagation_length << ", tolerance = " << tol << std::endl
                  << "\tBN (structure and starting parameters): " << net_file << std::endl
                  << "\tdata set (unlisted variables are missing): " << test_set_file << std::endl
                  << "===============================" << std::endl;
        auto die = [] {
            fprintf(stderr, "Error: %s\n", fbn_last_error());
            return 1;
        };
        fbn_network *net = nullptr;
        if (fbn_network_load_xmlbif(net_file.c_str(), &net)) return die();
        int n = 0;
        fbn_network_num_nodes(net, &n);
        TestSet tester;
        if (tester.Load(test_set_file, n)) return die();
        const int64_t nc = tester.num_instances();
        fbn_em *em = nullptr;
        if (fbn_em_create(net, device, &em)) return die();
        const int iters = propagation_length;
        std::vector<double> objective((size_t)(iters > 0 ? iters : 1) * 2);
        int done = 0;
        if (fbn_em_run(em, tester.evidence.data(), nc, iters, tol, 1.0, objective.data(), &done)) return die();
        std::cout << "cases = " << nc << std::endl;
        for (int t = 0; t < done; ++t) {
            char buf[128];
            snprintf(buf, sizeof buf, "iteration %d: log-likelihood = %.17g, Q = %.17g", t, objective[2 * t], objective[2 * t + 1]);
            std::cout << buf << std::endl;
        }
        float kms = 0.f;
        if (fbn_em_last_kernel_ms(em, &kms) == 0)  // not on the host path (--device -1)
            std::cout << "em: last E-step kernel " << kms * 1e-3 << " s, " << nc / (kms * 1e-3) << " cases/s" << std::endl;
        if (!out_file.empty()) {
            // one line per node and parent configuration: node, configuration, the probability of each state
            fbn_network *learned = nullptr;
            if (fbn_em_network(em, &learned)) return die();
            FILE *f = fopen(out_file.c_str(), "w");
            if (!f) {
                fprintf(stderr, "Error: cannot write %s\n", out_file.c_str());
                return 1;
            }
            std::vector<int32_t> dims(n);
            fbn_network_dims(learned, dims.data());
            for (int v = 0; v < n; ++v) {
                int npar = 0;
                int64_t np = 0;
                if (fbn_network_node_probs(learned, v, nullptr, nullptr, &npar, &np)) return die();
                std::vector<double> probs((size_t)np);
                if (fbn_network_node_probs(learned, v, nullptr, probs.data(), &npar, &np)) return die();
                const int64_t npc = np / dims[v];
                for (int64_t pc = 0; pc < npc; ++pc) {
                    fprintf(f, "%d %lld", v, (long long)pc);
                    for (int q = 0; q < dims[v]; ++q) fprintf(f, " %.17g", probs[(size_t)(q * npc + pc)]);
                    fprintf(f, "\n");
                }
            }
            fclose(f);
            fbn_network_destroy(learned);
            std::cout << "CPTs written to " << out_file << std::endl;
        }
        fbn_em_destroy(em);
        fbn_network_destroy(net);
    } else if (algorithm == 14 || algorithm == 17) {
        // score-based structure learning: no counterpart in the reference (its structure learner is PC-stable)
        const bool exact = algorithm == 17;
        std::cout << "===============================" << std::endl
                  << (exact ? "Algorithm: exact search (subset-lattice DP) for score-optimal structure learning, #threads = "
                            : "Algorithm: hill climbing (HC) for score-based structure learning, #threads = ")
                  << num_threads << std::endl
                  << "score = " << score_name << ", max parents = " << max_parents << std::endl
                  << "\tsample set: " << train_set_file << std::endl;
        if (ref_given) std::cout << "\treference BN: " << ref_net_file << std::endl;
        std::cout << "===============================" << std::endl;
        auto die = [] {
            fprintf(stderr, "Error: %s\n", fbn_last_error());
            return 1;
        };
        // the scores of continuous data (bic-g, aic-g, loglik-g: the Gaussian log-likelihood score; bge, with --iss as
        // alpha_mu) read -f2 as a CSV of reals, as -a 19 does, and go through the _gauss entries
        const bool gauss = IsGaussScore(score_name);
        if (gauss && exact) return RefuseGaussScore(score_name, algorithm);
        int n = 0;
        int64_t ns = 0;
        fbn_hc_options opt{};
        fbn_hc_result *res = nullptr;
        fbn_ci_ctx *ctx = nullptr;
        fbn_gci_ctx *gctx = nullptr;
        if (gauss) {
            fbn_cdataset *cds = nullptr;
            if (fbn_cdataset_load_csv(train_set_file.c_str(), &cds)) return die();
            fbn_cdataset_shape(cds, &n, &ns);
            std::vector<double> x((size_t)n * (size_t)ns);
            fbn_cdataset_columns(cds, x.data());
            fbn_cdataset_destroy(cds);
            fbn_gauss_score g{score_name == "bge" ? FBN_GSCORE_BGE : FBN_GSCORE_LL, 0, iss_given ? iss : 1.0, 0.0, 0.0};
            if (score_name != "bge") {
                if (iss_given) {
                    fprintf(stderr, "Error: --iss is alpha_mu of --score bge (or the equivalent sample size of bde); the score is %s\n",
                            score_name.c_str());
                    return 1;
                }
                if (fbn_hc_penalty(score_name.substr(0, score_name.size() - 2).c_str(), ns, &g.penalty)) return die();
            }
            opt.max_parents = max_parents;
            opt.max_iter = -1;
            if (device < 0) {
                // the host twin over moments formed here: centred sums of squares and the correlation matrix
                std::vector<double> ss((size_t)n), R((size_t)n * n);
                for (int v = 0; v < n; ++v) {
                    double *c = x.data() + (size_t)v * ns, m = 0.0;
                    for (int64_t i = 0; i < ns; ++i) m += c[i];
                    m /= (double)ns;
                    for (int64_t i = 0; i < ns; ++i) c[i] -= m;
                }
                for (int u = 0; u < n; ++u)
                    for (int v = u; v < n; ++v) {
                        const double *a = x.data() + (size_t)u * ns, *b = x.data() + (size_t)v * ns;
                        double d = 0.0;
                        for (int64_t i = 0; i < ns; ++i) d += a[i] * b[i];
                        R[(size_t)u * n + v] = R[(size_t)v * n + u] = d;
                    }
                for (int v = 0; v < n; ++v) ss[(size_t)v] = R[(size_t)v * n + v];
                for (int u = 0; u < n; ++u)
                    for (int v = 0; v < n; ++v) R[(size_t)u * n + v] = u == v ? 1.0 : R[(size_t)u * n + v] / sqrt(ss[(size_t)u] * ss[(size_t)v]);
                if (fbn_hc_run_gauss_host(n, ns, ss.data(), R.data(), &opt, &g, &res)) return die();
            } else if (fbn_gci_upload(x.data(), n, ns, device, &gctx) || fbn_hc_run_gauss(gctx, &opt, &g, &res)) {
                return die();
            }
        } else {
            DiscreteSet D;
            if (!LoadDiscreteSet(train_set_file, &D)) return die();
            n = D.n, ns = D.ns;
            LearnerScore sc;
            if (ParseLearnerScore(score_name, iss_given, iss, ns, &sc)) return 1;
            opt.penalty = sc.penalty;
            opt.max_parents = max_parents;
            opt.max_iter = -1;
            fbn_exact_options xopt{};
            xopt.penalty = opt.penalty;
            xopt.max_parents = max_parents;
            if (device < 0) {
                if (sc.is_bd ? (exact ? fbn_exact_run_bd_host(n, D.dims.data(), D.cols.data(), ns, &xopt, &sc.bd, &res)
                                   : fbn_hc_run_bd_host(n, D.dims.data(), D.cols.data(), ns, &opt, &sc.bd, &res))
                          : (exact ? fbn_exact_run_host(n, D.dims.data(), D.cols.data(), ns, &xopt, &res)
                                   : fbn_hc_run_host(n, D.dims.data(), D.cols.data(), ns, &opt, &res)))
                    return die();
            } else {
                if (fbn_ci_dataset_upload(D.cols.data(), n, ns, D.dims.data(), device, &ctx)) return die();
                if (sc.is_bd ? (exact ? fbn_exact_run_bd(ctx, &xopt, &sc.bd, &res) : fbn_hc_run_bd(ctx, &opt, &sc.bd, &res))
                          : (exact ? fbn_exact_run(ctx, &xopt, &res) : fbn_hc_run(ctx, &opt, &res)))
                    return die();
            }
        }
        fbn_hc_info info;
        fbn_hc_result_info(res, &info);
        std::vector<int32_t> off((size_t)n + 1), par((size_t)(info.narcs > 0 ? info.narcs : 1));
        fbn_hc_result_parents(res, off.data(), par.data());
        char buf[160];
        std::cout << "variables = " << n << ", samples = " << ns << std::endl << "arcs = " << info.narcs << std::endl;
        snprintf(buf, sizeof buf, "score = %.17g, log-likelihood = %.17g", info.score, info.loglik);
        std::cout << buf << std::endl;
        if (exact) {
            fbn_exact_info x;
            fbn_exact_result_info(res, &x);
            std::cout << "exact: " << x.families_scored << " families scored in " << x.batches << " batches, " << x.lattice_bytes
                      << " lattice bytes, " << x.passes << " transform passes; device kernel: scores " << x.score_kernel_ms * 1e-3
                      << " s, transform " << x.transform_kernel_ms * 1e-3 << " s, sinks " << x.sink_kernel_ms * 1e-3 << " s; search "
                      << x.wall_ms * 1e-3 << " s" << std::endl;
        } else {
            std::cout << "iterations = " << info.iterations << std::endl;
            std::cout << "hc: " << info.families_scored << " families scored in " << info.batches << " batches, device kernel "
                      << info.kernel_ms * 1e-3 << " s, search " << info.wall_ms * 1e-3 << " s" << std::endl;
        }
        if (ref_given) {
            std::vector<int32_t> tri;
            for (int v = 0; v < n; ++v)
                for (int32_t k = off[v]; k < off[v + 1]; ++k) tri.insert(tri.end(), {par[k], v, 1});
            int shd = 0;
            if (fbn_shd_bif(ref_net_file.c_str(), n, tri.data(), info.narcs, &shd)) return die();
            std::cout << "SHD = " << shd << std::endl;
        }
        if (!out_file.empty()) {
            FILE *f = fopen(out_file.c_str(), "w");
            if (!f) {
                fprintf(stderr, "Error: cannot write %s\n", out_file.c_str());
                return 1;
            }
            for (int v = 0; v < n; ++v) {
                fprintf(f, "%d %d", v, off[v + 1] - off[v]);
                for (int32_t k = off[v]; k < off[v + 1]; ++k) fprintf(f, " %d", par[k]);
                fprintf(f, "\n");
            }
            fclose(f);
            std::cout << "DAG written to " << out_file << std::endl;
        }
        fbn_hc_result_destroy(res);
        if (ctx) fbn_ci_ctx_destroy(ctx);
        if (gctx) fbn_gci_ctx_destroy(gctx);
    } else if (algorithm == 18) {
        // exact arc posteriors: no counterpart in the reference
        std::cout << "===============================" << std::endl
                  << "Algorithm: exact arc posteriors (Bayesian model averaging on the subset lattice), #threads = " << num_threads
                  << std::endl
                  << "score = " << score_name << ", max parents = " << max_parents << ", prior = " << prior_name << std::endl
                  << "\tsample set: " << train_set_file << std::endl
                  << "===============================" << std::endl;
        if (IsGaussScore(score_name)) return RefuseGaussScore(score_name, algorithm);
        auto die = [] {
            fprintf(stderr, "Error: %s\n", fbn_last_error());
            return 1;
        };
        if (prior_name != "uniform" && prior_name != "indegree") {
            fprintf(stderr, "Error: --prior is uniform or indegree, not %s\n", prior_name.c_str());
            return 1;
        }
        const int32_t prior = prior_name == "indegree";
        DiscreteSet D;
        if (!LoadDiscreteSet(train_set_file, &D)) return die();
        const int n = D.n;
        const int64_t ns = D.ns;
        LearnerScore sc;
        if (ParseLearnerScore(score_name, iss_given, iss, ns, &sc)) return 1;
        fbn_exact_options xopt{};
        xopt.penalty = sc.penalty;
        xopt.max_parents = max_parents;
        fbn_bma_result *res = nullptr;
        fbn_ci_ctx *ctx = nullptr;
        if (device < 0) {
            if (sc.is_bd ? fbn_bma_run_bd_host(n, D.dims.data(), D.cols.data(), ns, &xopt, prior, &sc.bd, &res)
                      : fbn_bma_run_host(n, D.dims.data(), D.cols.data(), ns, &xopt, prior, &res))
                return die();
        } else {
            if (fbn_ci_dataset_upload(D.cols.data(), n, ns, D.dims.data(), device, &ctx)) return die();
            if (sc.is_bd ? fbn_bma_run_bd(ctx, &xopt, prior, &sc.bd, &res) : fbn_bma_run(ctx, &xopt, prior, &res)) return die();
        }
        fbn_bma_info info;
        fbn_bma_result_info(res, &info);
        std::vector<double> P((size_t)n * (size_t)n);
        fbn_bma_result_arcs(res, P.data(), nullptr);
        char buf[160];
        std::cout << "variables = " << n << ", samples = " << ns << std::endl;
        snprintf(buf, sizeof buf, "logZ = %.17g, B[V] = %.17g", info.log_z, info.b_full);
        std::cout << buf << std::endl << "arcs with posterior >= 0.5:" << std::endl;
        for (int u = 0; u < n; ++u)
            for (int v = 0; v < n; ++v)
                if (P[(size_t)u * n + v] >= 0.5) {
                    snprintf(buf, sizeof buf, "%d -> %d %.17g", u, v, P[(size_t)u * n + v]);
                    std::cout << buf << std::endl;
                }
        std::cout << "bma: " << info.families_scored << " families scored in " << info.batches << " batches, " << info.lattice_bytes
                  << " lattice bytes, " << info.passes << " passes per transform; device kernel: scores " << info.score_kernel_ms * 1e-3
                  << " s, alpha " << info.alpha_kernel_ms * 1e-3 << " s, levels " << info.level_kernel_ms * 1e-3 << " s, Gamma "
                  << info.gamma_kernel_ms * 1e-3 << " s, q " << info.q_kernel_ms * 1e-3 << " s; total " << info.wall_ms * 1e-3 << " s"
                  << std::endl;
        if (!out_file.empty()) {
            FILE *f = fopen(out_file.c_str(), "w");
            if (!f) {
                fprintf(stderr, "Error: cannot write %s\n", out_file.c_str());
                return 1;
            }
            for (int u = 0; u < n; ++u)
                for (int v = 0; v < n; ++v) fprintf(f, "%.17g%c", P[(size_t)u * n + v], v + 1 < n ? ' ' : '\n');
            fclose(f);
            std::cout << "arc posteriors written to " << out_file << std::endl;
        }
        fbn_bma_result_destroy(res);
        if (ctx) fbn_ci_ctx_destroy(ctx);
    } else if (algorithm == 20) {
        // order MCMC: no counterpart in the reference
        const long long chains = q_given ? num_samples : 64, burn_in = m_given ? max_updating : 2000,
                        samples = l_given ? updating_interval : 200;
        if (max_parents < 0) max_parents = 3;
        std::cout << "===============================" << std::endl
                  << "Algorithm: arc posteriors by MCMC over node orders, #threads = " << num_threads << std::endl
                  << "score = " << score_name << ", max parents = " << max_parents << ", prior = " << prior_name << std::endl
                  << "chains = " << chains << ", burn-in = " << burn_in << ", samples = " << samples << ", thin = " << thin
                  << ", seed = " << seed << std::endl
                  << "\tsample set: " << train_set_file << std::endl
                  << "===============================" << std::endl;
        if (IsGaussScore(score_name)) return RefuseGaussScore(score_name, algorithm);
        auto die = [] {
            fprintf(stderr, "Error: %s\n", fbn_last_error());
            return 1;
        };
        if (prior_name != "uniform" && prior_name != "indegree") {
            fprintf(stderr, "Error: --prior is uniform or indegree, not %s\n", prior_name.c_str());
            return 1;
        }
        if (chains < 1 || chains > 0x7fffffffLL || samples < 1 || samples > 0x7fffffffLL) {
            fprintf(stderr, "Error: -q chains and -l samples are 1 .. 2^31 - 1\n");
            return 1;
        }
        const int32_t prior = prior_name == "indegree";
        DiscreteSet D;
        if (!LoadDiscreteSet(train_set_file, &D)) return die();
        const int n = D.n;
        const int64_t ns = D.ns;
        LearnerScore sc;
        if (ParseLearnerScore(score_name, iss_given, iss, ns, &sc)) return 1;
        fbn_exact_options xopt{};
        xopt.penalty = sc.penalty;
        xopt.max_parents = max_parents;
        const fbn_omcmc_options mopt{(int32_t)chains, (int32_t)samples, burn_in, thin, seed, 0, 0};
        fbn_omcmc_result *res = nullptr;
        fbn_ci_ctx *ctx = nullptr;
        if (device < 0) {
            if (sc.is_bd ? fbn_omcmc_run_bd_host(n, D.dims.data(), D.cols.data(), ns, &xopt, prior, &sc.bd, &mopt, &res)
                      : fbn_omcmc_run_host(n, D.dims.data(), D.cols.data(), ns, &xopt, prior, &mopt, &res))
                return die();
        } else {
            if (fbn_ci_dataset_upload(D.cols.data(), n, ns, D.dims.data(), device, &ctx)) return die();
            if (sc.is_bd ? fbn_omcmc_run_bd(ctx, &xopt, prior, &sc.bd, &mopt, &res) : fbn_omcmc_run(ctx, &xopt, prior, &mopt, &res)) return die();
        }
        fbn_omcmc_info info;
        fbn_omcmc_result_info(res, &info);
        const size_t nn = (size_t)n * (size_t)n;
        std::vector<double> P(nn), PC((size_t)chains * nn);
        std::vector<int64_t> accepted((size_t)chains);
        fbn_omcmc_result_arcs(res, P.data(), PC.data(), nullptr, nullptr, accepted.data());
        char buf[160];
        std::cout << "variables = " << n << ", samples = " << ns << std::endl << "arcs with posterior >= 0.5:" << std::endl;
        for (int u = 0; u < n; ++u)
            for (int v = 0; v < n; ++v)
                if (P[(size_t)u * n + v] >= 0.5) {
                    snprintf(buf, sizeof buf, "%d -> %d %.17g", u, v, P[(size_t)u * n + v]);
                    std::cout << buf << std::endl;
                }
        double acc_sum = 0.0, se_max = 0.0;
        for (long long c = 0; c < chains; ++c) acc_sum += (double)accepted[(size_t)c];
        for (size_t e = 0; chains > 1 && e < nn; ++e) {  // the chains are independent: sd / sqrt(chains)
            double ss = 0.0;
            for (long long c = 0; c < chains; ++c) ss += (PC[(size_t)c * nn + e] - P[e]) * (PC[(size_t)c * nn + e] - P[e]);
            se_max = std::max(se_max, std::sqrt(ss / (double)(chains - 1) / (double)chains));
        }
        snprintf(buf, sizeof buf, "acceptance rate = %.6g, largest standard error of an arc = %.6g", acc_sum / ((double)chains * (double)info.steps),
                 se_max);
        std::cout << buf << std::endl;
        std::cout << "omcmc: " << info.families << " families in the lists (" << info.family_bytes << " bytes), scored in " << info.batches
                  << " batches; " << info.steps << " steps per chain in " << info.launches << " launches; device kernel: scores "
                  << info.score_kernel_ms * 1e-3 << " s, chains " << info.chain_kernel_ms * 1e-3 << " s; total " << info.wall_ms * 1e-3 << " s"
                  << std::endl;
        if (!out_file.empty()) {
            FILE *f = fopen(out_file.c_str(), "w");
            if (!f) {
                fprintf(stderr, "Error: cannot write %s\n", out_file.c_str());
                return 1;
            }
            for (int u = 0; u < n; ++u)
                for (int v = 0; v < n; ++v) fprintf(f, "%.17g%c", P[(size_t)u * n + v], v + 1 < n ? ' ' : '\n');
            fclose(f);
            std::cout << "arc posteriors written to " << out_file << std::endl;
        }
        fbn_omcmc_result_destroy(res);
        if (ctx) fbn_ci_ctx_destroy(ctx);
    } else if (algorithm == 19) {
        // PC-stable on continuous data: no counterpart in the reference (its ContinuousNode has no learner)
        std::cout << "===============================" << std::endl
                  << "Algorithm: PC-stable on continuous data (Fisher-z partial correlation), #threads = " << num_threads << std::endl
                  << "\tsample set: " << train_set_file << std::endl;
        if (ref_given) std::cout << "\treference BN: " << ref_net_file << std::endl;
        std::cout << "===============================" << std::endl;
        auto die = [] {
            fprintf(stderr, "Error: %s\n", fbn_last_error());
            return 1;
        };
        fbn_cdataset *ds = nullptr;
        if (fbn_cdataset_load_csv(train_set_file.c_str(), &ds)) return die();
        int n = 0;
        int64_t ns = 0;
        fbn_cdataset_shape(ds, &n, &ns);
        std::vector<double> cols((size_t)n * (size_t)ns);
        fbn_cdataset_columns(ds, cols.data());
        fbn_cdataset_destroy(ds);
        std::cout << "==================================================" << '\n'
                  << "Begin structural learning with PC-stable" << std::endl;
        fbn_gci_ctx *ctx = nullptr;
        fbn_pc_result *res = nullptr;
        if (fbn_gci_upload(cols.data(), n, ns, device, &ctx) || fbn_gci_pc_stable(ctx, 0.05, depth, &res)) return die();
        int nl = 0, ne = 0, no = 0;
        fbn_pc_num_levels(res, &nl);
        std::vector<int64_t> tests((size_t)nl);
        fbn_pc_level_tests(res, tests.data());
        int64_t total = 0;
        for (int l = 0; l < nl; ++l) {
            total += tests[l];
            std::cout << "Level " << l << "... # of CI-tests is " << total << std::endl;
        }
        fbn_pc_num_edges(res, &ne);
        double total_s = 0, kernel_s = 0, min_margin = 0;
        int64_t near = 0, degenerate = 0;
        float corr_ms[3] = {0.f, 0.f, 0.f};
        fbn_pc_timing(res, &total_s, &kernel_s);
        fbn_pc_decision_margin(res, &min_margin, &near);
        fbn_pc_degenerate(res, &degenerate);
        fbn_gci_corr_kernel_ms(ctx, corr_ms);
        std::cout << "==================================================" << std::endl;
        std::cout << "# of CI-tests is " << total << ", # of degenerate tests is " << degenerate << std::endl;
        std::cout << "# remaining edges = " << ne << std::endl;
        std::cout << "correlation: device kernels " << (corr_ms[0] + corr_ms[1] + corr_ms[2]) * 1e-3 << " s; pc-stable step 1: "
                  << total_s << " s (device kernels " << kernel_s << " s)" << std::endl;
        std::cout << "min | |r| - tau | = " << min_margin << " (" << near << " decisions within 1e-9)" << std::endl;
        fbn_pc_num_oriented_edges(res, &no);
        std::vector<int32_t> tri(3 * (size_t)no + 3);
        fbn_pc_oriented_edges(res, tri.data());
        if (ref_given) {
            int shd = 0;
            if (fbn_shd_bif(ref_net_file.c_str(), n, tri.data(), no, &shd)) return die();
            std::cout << "SHD = " << shd << std::endl;
        }
        if (!out_file.empty()) {
            // one line per edge of the learned PDAG: from, to, 1 for an arc; min, max, 0 for an undirected edge
            FILE *f = fopen(out_file.c_str(), "w");
            if (!f) {
                fprintf(stderr, "Error: cannot write %s\n", out_file.c_str());
                return 1;
            }
            for (int e = 0; e < no; ++e) fprintf(f, "%d %d %d\n", tri[3 * e], tri[3 * e + 1], tri[3 * e + 2]);
            fclose(f);
            std::cout << "PDAG written to " << out_file << std::endl;
        }
        fbn_pc_result_destroy(res);
        fbn_gci_ctx_destroy(ctx);
    } else if (algorithm == 15) {
        // exact posterior sampling: no counterpart in the reference (its samplers weigh; none draws from P(x | e))
        std::cout << "===============================" << std::endl
                  << "Algorithm: exact posterior sampling on the junction forest, #threads = " << num_threads << std::endl
                  << "number of samples = " << num_samples << ", seed = " << seed << std::endl
                  << "\tBN: " << net_file << std::endl
                  << "\ttesting set: " << test_set_file << std::endl
                  << "===============================" << std::endl;
        auto die = [] {
            fprintf(stderr, "Error: %s\n", fbn_last_error());
            return 1;
        };
        fbn_network *net = nullptr;
        if (fbn_network_load_xmlbif(net_file.c_str(), &net)) return die();
        int n = 0;
        fbn_network_num_nodes(net, &n);
        TestSet tester;
        if (tester.Load(test_set_file, n)) return die();
        const int64_t nc = tester.num_instances(), S = num_samples;
        fbn_psample *ps = nullptr;
        if (fbn_psample_create(net, device, &ps)) return die();
        std::vector<int8_t> rows((size_t)nc * (size_t)(S > 0 ? S : 0) * n);
        std::vector<double> value((size_t)nc * 2);
        if (fbn_psample_run(ps, tester.evidence.data(), nc, S, seed, 0, rows.data(), value.data())) return die();
        float kms = 0.f;
        const bool timed = fbn_psample_last_kernel_ms(ps, &kms) == 0;  // not on the host path (--device -1)
        double sum = 0;
        for (int64_t c = 0; c < nc; ++c) sum += log(value[2 * c]) + value[2 * c + 1] * log(2.0);
        std::cout << "cases = " << nc << std::endl;
        char buf[64];
        snprintf(buf, sizeof buf, "%.12g", nc ? sum / nc : 0.0);
        std::cout << "average log P(e) = " << buf << std::endl;
        if (timed)
            std::cout << "psample: device kernel " << kms * 1e-3 << " s, " << (double)nc * S / (kms * 1e-3) << " samples/s"
                      << std::endl;
        if (!out_file.empty()) {
            // S consecutive rows per case; label = the value of variable 0
            std::vector<int32_t> labels((size_t)(nc * S));
            for (int64_t r = 0; r < nc * S; ++r) labels[r] = rows[(size_t)r * n];
            if (fbn_write_libsvm(out_file.c_str(), rows.data(), nc * S, n, labels.data())) return die();
            std::cout << "samples written to " << out_file << std::endl;
        }
        fbn_psample_destroy(ps);
        fbn_network_destroy(net);
    } else if (algorithm == 16) {
        // Gibbs sampling: no counterpart in the reference; -a 10's result lines
        std::cout << "===============================" << std::endl
                  << "Algorithm: Gibbs sampling for approximate inference, #threads = " << num_threads << std::endl
                  << "chains = " << num_samples << ", burn-in sweeps = " << max_updating << ", counted sweeps = " << updating_interval
                  << ", seed = " << seed << std::endl
                  << "\tBN: " << net_file << std::endl
                  << "\ttesting set: " << test_set_file << std::endl
                  << "\treference potential table: " << pt_file << std::endl
                  << "===============================" << std::endl;
        auto die = [] {
            fprintf(stderr, "Error: %s\n", fbn_last_error());
            return 1;
        };
        fbn_network *net = nullptr;
        if (fbn_network_load_xmlbif(net_file.c_str(), &net)) return die();
        int n = 0;
        fbn_network_num_nodes(net, &n);
        TestSet tester;
        if (tester.Load(test_set_file, n)) return die();
        const int64_t nc = tester.num_instances();
        std::vector<int32_t> dims(n);
        fbn_network_dims(net, dims.data());
        int sum_dom = 0;
        for (int d : dims) sum_dom += d;
        std::vector<double> golden = LoadGroundTruth(pt_file, dims, nc);
        std::cout << "==================================================" << '\n'
                  << "Begin testing the trained network." << std::endl;
        fbn_gibbs *gs = nullptr;
        if (fbn_gibbs_create(net, device, &gs)) return die();
        std::vector<int32_t> predictions((size_t)nc);
        std::vector<double> marginals((size_t)nc * sum_dom);
        if (fbn_gibbs_run(gs, tester.evidence.data(), nc, num_samples, max_updating, updating_interval, seed, 0,
                          predictions.data(), marginals.data(), nullptr))
            return die();
        float kms = 0.f;
        const bool timed = fbn_gibbs_last_kernel_ms(gs, &kms) == 0;  // not on the host path (--device -1)
        double mse = 0, hd = 0;
        if (fbn_score_marginals(net, marginals.data(), golden.data(), nc, &mse, &hd)) return die();
        int64_t correct = 0;
        for (int64_t c = 0; c < nc; ++c) correct += predictions[c] == tester.ground_truths[c];
        std::cout << "average MSE = " << mse / nc << std::endl;
        std::cout << "average HD = " << hd / nc << std::endl;
        std::cout << "==================================================" << std::endl;
        if (timed)
            std::cout << "gibbs: device kernel " << kms * 1e-3 << " s, "
                      << (double)nc * (double)num_samples * (double)(max_updating + updating_interval) / (kms * 1e-3)
                      << " chain-sweeps/s" << std::endl;
        std::cout << "accuracy = " << correct / (double)nc << std::endl;
        fbn_gibbs_destroy(gs);
        fbn_network_destroy(net);
    } else if (algorithm == 9) {
        // SISv1 (ALGSISV1, src/main.cpp:162-173): the reference names it and defines it nowhere, in code or papers
        std::cout << "SISv1 is not defined by the reference (no code, no paper): not built.  Use -a 8 (SIS) or -a 10 (AIS-BN)."
                  << std::endl;
    } else if (algorithm >= 0 && algorithm <= 11) {
        std::cout << "This algorithm is not on the accelerated path of this build (only -a 0, 2, 4, 5, 6, 7, 8, 10, 12, 13, 14, 15, 16, 17, 18, 19 and 20)." << std::endl;
    } else {
        std::cout << "\tError! Please give the right value of -a to specify the functionality/algorithm" << std::endl;
    }
    return 0;
}
