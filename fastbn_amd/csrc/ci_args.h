// ci_args.h -- the argument records of the CI kernels' launchers (launchers.h): what capi_ci.hip and
// capi_pc.hip fill, field by field, and ci_kernels.hip / ci_bits_*.hip / ci_l1.hip read.  CiArgs,
// CiG2Args and CiL1Args are also by-value kernel parameters (the histogram kernel, the bit-sliced
// G^2 passes, the level-1 setup and resolve); CiBitsArgs is host-only.  Internal to libfastbn.
#ifndef FBN_CI_ARGS_H
#define FBN_CI_ARGS_H

#include <stdint.h>

// ci_g2_kernel's parameter: field order and types are the kernarg layout
struct CiArgs {
    const uint8_t *cols;  // [nvars][N]
    const int32_t *dims;
    const int32_t *items;  // [n][2+D]
    long long N;
    long long n;
    double alpha;
    double *g2;
    int32_t *df;
    double *p;
    uint8_t *indep;
    int32_t *counts;  // optional: histogram of item 0
    int32_t *gscratch;  // non-null: tables too large for LDS live in global memory, one region per
    long long gstride;  // workgroup of gstride ints (same layout as the LDS one; set by fbn_ci_launch)
    // decision-margin log: [0] = min over tests of |p - alpha| as IEEE bits
    // (non-negative doubles order like their bit patterns), [1] = #tests with |p - alpha| < 1e-9
    unsigned long long *stats;
    // non-null: count from the bit-sliced store instead (every variable of every test has <= 4
    // states; all value rows of variable v start at row0[v], W words per row)
    const uint32_t *bits;
    const int32_t *row0;
    long long W;
    // decisions only (p == nullptr): [lo, hi] per df 1..nband then delta (ci_chisq.h fbn_chisq_band)
    const double *band;
    int nband;
    // PK instantiation: the columns packed 2 bits per sample (every state count <= 4), 16 samples
    // per word, PW words per variable (fbn_ci_pack2_build)
    const uint32_t *pk;
    long long PW;
    // counts != nullptr: cstride == 0 -> the table of test 0 only; cstride > 0 -> every test's table
    // at counts + test * cstride (fbn_ci_debug_counts)
    long long cstride;
    // split mode (small batches, MODE 1 / 2): test t's table at tab + t * tstride (zeroed), its
    // packed words divided among `split` workgroups
    int32_t *tab;
    long long tstride;
    int split;
    // MODE 3 (d = 2, bit-sliced, derived): the pair tables of this PC run's level 0 (every pair u < v
    // of the nvars variables, [value of u][value of v], ci_bits_count.hip pair_table)
    const int32_t *pairtab;
    int nvars;
    int dbg;  // diagnostic ablations, 0 from every launcher: bit 0 = MODE 3 skips its counting
};

// fbn_ci_bits_launch: n tests with d <= 1 conditioning variables from the bit-sliced store
struct CiBitsArgs {
    const uint32_t *bits;
    const int32_t *dims;
    const int32_t *row0;
    const int32_t *rowcnt;  // samples per mask row
    const int32_t *items;   // [n][2+d]; null: test t is pair t0 + t of the complete graph
    long long W, n, t0;
    int d;
    double alpha;
    double *g2;  // optional outputs: g2, p, counts0
    int32_t *df;
    double *p;
    uint8_t *indep;
    int32_t *counts;   // [n][64], every test's table (scratch of the two kernels)
    int32_t *counts0;  // the table of test 0 (fbn_ci_counts)
    unsigned long long *stats;
    int32_t *pairtab;  // pmode 1: recorded here (d = 0); pmode 2: read (d = 1); pmode 0: unused
    int pmode;
    int nvars, num_cu;
    int counted;  // d = 0: the counts are already in place (Gram or tiled pairs), only decide
    const double *band;
    int nband;
};

// ci_bits_g2 / ci_bits_g2q's parameter (ci_bits_g2.hip): the G^2 pass over n count records
struct CiG2Args {
    const int32_t *counts;  // [n][64]
    const int32_t *dims;
    const int32_t *items;  // [n][2+d]; null (d = 0): test t is pair t0 + t of the complete graph over nvars
    long long n, t0;
    int nvars;
    double alpha;
    double *g2;  // optional outputs: g2, p, counts0 (the table of test 0)
    int32_t *df;
    double *p;
    uint8_t *indep;
    int32_t *counts0;
    unsigned long long *stats;  // optional: the decision-margin log
    const double *band;         // optional, used when p == nullptr
    int nband;
    const long long *n_dev;  // non-null: the test count is read on the device (batches generated there)
};

// fbn_ci_l1_setup and fbn_ci_l1_round: the device-resident level-1 search.  Filled once per level;
// what changes per round (open_cnt, open_next, next_chunk, epoch) is passed beside it.  Also the
// parameter of ci_l1_setup and ci_l1_resolve (ci_l1.hip).
struct CiL1Args {
    // the level's edges and adjacency (CSR)
    const int32_t *pairs;
    const int32_t *adj, *adj_off;
    int E, nv, num_cu;
    // per-edge search state
    void *ed;
    int32_t *pos;
    uint8_t *st;
    int32_t *sep;
    long long *counted;
    int32_t *len, *off;
    unsigned *ring;             // the open-count ring, zeroed by the setup
    unsigned long long *sstat;  // tile-scan status words
    long long *scal;            // total, launched, rows read, scan flag, tickets
    long long cap;              // tests a round may hold
    int chunk0;                 // round 0's per-edge chunk
    // a round's tests
    const uint32_t *bits;
    const int32_t *dims, *row0;
    long long W;
    const int32_t *pairtab;
    int32_t *items, *counts, *df;
    uint8_t *indep;
    double alpha;
    unsigned long long *stats;
    const double *band;
    int nband;
    // the information screen: mi = every pair's level-0 G^2 (null: no screen; computed by the setup
    // from the pair tables when mi_from_tables), two_n = 2N, pcnt >= E ints, plist >= the level's
    // candidate sets (null without the screen), sstat2 / scal2 a second tile-status array and 4 scalars
    double *mi;
    int mi_from_tables;
    double two_n;
    int32_t *pcnt, *plist;
    unsigned long long *sstat2;
    long long *scal2;
};

#endif
