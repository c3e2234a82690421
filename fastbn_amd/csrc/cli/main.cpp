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
// deletions and reversals from the empty graph on -f2's CSV (--score bic|aic|loglik, default bic;
// --max-parents K); prints the arc count, the score and the iterations, and with -f1 given the SHD against
// that network through -a 0's comparison; --out FILE writes the DAG, one line per node: node, number of
// parents, parents ascending.  --device -1 runs the host twin (same result, bit for bit).
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

int main(int argc, char **argv) {
    int algorithm = 2, num_threads = 1, group_size = 1, device = 0, depth = 1000, gpus = 1, propagation_length = 2;
    double tol = 0.0, damping = 0.0, eps = -1.0;
    long long num_samples = 10000, max_updating = 10, updating_interval = 2500;  // src/Parameter.cpp:14-15
    unsigned long long seed = 0;
    std::string out_file, score_name = "bic";
    int max_parents = -1;
    bool ref_given = false;
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
        if (a == "--max-parents" && i + 1 < argc) { max_parents = atoi(argv[++i]); continue; }
        switch (argv[i][1]) {
        case 'h':
            std::cout << "Usage: ./BayesianNetwork [-a 0|2|4|5|6|7|8|10|12|13|14] [-t threads] [-g group] [-q samples] [-d length] [-m updates] "
                         "[-l interval] [-f0 net] "
                         "[-f1 refnet] [-f2 train] [-f3 test] [-f4 pt] [--device N] [--gpus G] [--depth D] [--seed N] "
                         "[--tol T] [--damping L] [--eps E] [--score bic|aic|loglik] [--max-parents K] [--out FILE] [--prefix DIR]"
                      << std::endl;
            return 0;
        case 'a': algorithm = atoi(argv[++i]); break;
        case 't': num_threads = atoi(argv[++i]); break;
        case 'g': group_size = atoi(argv[++i]); break;
        case 'q': num_samples = atoll(argv[++i]); break;
        case 'd': propagation_length = atoi(argv[++i]); break;  // src/Parameter.cpp:40
        case 'm': max_updating = atoll(argv[++i]); break;       // src/Parameter.cpp:38
        case 'l': updating_interval = atoll(argv[++i]); break;  // src/Parameter.cpp:39
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
    } else if (algorithm == 14) {
        // score-based structure learning: no counterpart in the reference (its structure learner is PC-stable)
        std::cout << "===============================" << std::endl
                  << "Algorithm: hill climbing (HC) for score-based structure learning, #threads = " << num_threads << std::endl
                  << "score = " << score_name << ", max parents = " << max_parents << std::endl
                  << "\tsample set: " << train_set_file << std::endl;
        if (ref_given) std::cout << "\treference BN: " << ref_net_file << std::endl;
        std::cout << "===============================" << std::endl;
        auto die = [] {
            fprintf(stderr, "Error: %s\n", fbn_last_error());
            return 1;
        };
        fbn_dataset *ds = nullptr;
        if (fbn_dataset_load_csv(train_set_file.c_str(), &ds)) return die();
        int n = 0;
        int64_t ns = 0;
        fbn_dataset_shape(ds, &n, &ns);
        std::vector<int32_t> dims((size_t)n);
        std::vector<uint8_t> cols((size_t)n * (size_t)ns);
        fbn_dataset_dims(ds, dims.data());
        fbn_dataset_columns(ds, cols.data());
        fbn_dataset_destroy(ds);
        fbn_hc_options opt{};
        if (fbn_hc_penalty(score_name.c_str(), ns, &opt.penalty)) return die();
        opt.max_parents = max_parents;
        opt.max_iter = -1;
        fbn_hc_result *res = nullptr;
        fbn_ci_ctx *ctx = nullptr;
        if (device < 0) {
            if (fbn_hc_run_host(n, dims.data(), cols.data(), ns, &opt, &res)) return die();
        } else {
            if (fbn_ci_dataset_upload(cols.data(), n, ns, dims.data(), device, &ctx)) return die();
            if (fbn_hc_run(ctx, &opt, &res)) return die();
        }
        fbn_hc_info info;
        fbn_hc_result_info(res, &info);
        std::vector<int32_t> off((size_t)n + 1), par((size_t)(info.narcs > 0 ? info.narcs : 1));
        fbn_hc_result_parents(res, off.data(), par.data());
        char buf[160];
        std::cout << "variables = " << n << ", samples = " << ns << std::endl << "arcs = " << info.narcs << std::endl;
        snprintf(buf, sizeof buf, "score = %.17g, log-likelihood = %.17g", info.score, info.loglik);
        std::cout << buf << std::endl << "iterations = " << info.iterations << std::endl;
        std::cout << "hc: " << info.families_scored << " families scored in " << info.batches << " batches, device kernel "
                  << info.kernel_ms * 1e-3 << " s, search " << info.wall_ms * 1e-3 << " s" << std::endl;
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
    } else if (algorithm == 9) {
        // SISv1 (ALGSISV1, src/main.cpp:162-173): the reference names it and defines it nowhere, in code or papers
        std::cout << "SISv1 is not defined by the reference (no code, no paper): not built.  Use -a 8 (SIS) or -a 10 (AIS-BN)."
                  << std::endl;
    } else if (algorithm >= 0 && algorithm <= 11) {
        std::cout << "This algorithm is not on the accelerated path of this build (only -a 0, 2, 4, 5, 6, 7, 8, 10, 12, 13 and 14)." << std::endl;
    } else {
        std::cout << "\tError! Please give the right value of -a to specify the functionality/algorithm" << std::endl;
    }
    return 0;
}
