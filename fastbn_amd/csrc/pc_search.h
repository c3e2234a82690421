// pc_search.h -- one level (d >= 1) of the PC-stable skeleton search without a device: which tests
// each round holds and what their answers mean.  The caller (RunLevel, pc_driver.cpp; or
// tools/pc_search_host_check.cpp) runs the tests and hands the decisions back.
//
// Instead of the reference's 128-edge work pool, every unresolved edge contributes its next chunk of
// candidate sets to one batch per round (first chunk sized so one round holds ~8k tests, at most 32
// per edge; then x growth per round), and each edge's prefix is resolved in order.  Tests beyond an
// edge's first independent set are speculative: generated but not counted, so the counts equal the
// reference's.  The semantics are in pc_driver.cpp's header.
#ifndef FBN_PC_SEARCH_H
#define FBN_PC_SEARCH_H

#include "pc_internal.h"

namespace fbn {

constexpr int kMaxD = 8;  // CI tests take at most 8 conditioning variables (capi_ci.hip)
constexpr int64_t kPipelineEdges = 2048;

struct SearchSchedule {
    int64_t round0 = 8192;      // tests the first round aims at: chunk = min(32, round0 / open edges)
    int64_t growth = 4;         // chunk factor per round (at least 2)
    int64_t full_spec = 16384;  // a level of at most this many candidate sets runs in a single round
    int64_t pipeline_edges = kPipelineEdges;  // a level of several rounds with fewer open edges runs as one half
    int64_t split_full = 4096;  // a single-round level splits into two halves from this many sets
    bool general = false;       // the general generator also at d = 1, group size 1
};

class LevelSearch {
  public:
    // the edges [e_begin, e_end) of sk against sk's adjacency; dims: state count per variable
    LevelSearch(const Skeleton &sk, size_t e_begin, size_t e_end, int d, int group_size, const int32_t *dims,
                const SearchSchedule &sch);
    // Two halves of the edge range, each with its own rounds, alternate on the device: while one
    // half's batch runs, the host resolves the other's results and generates its next round.  One half
    // when the level is small.
    int halves() const { return nh_; }
    // half h's next round: tests(h) tests of 2 + d variables each in items(h), their statistics in
    // stats(h); false when the half has nothing left
    bool Generate(int h);
    const std::vector<int32_t> &items(int h) const { return H_[h].items; }
    int64_t tests(int h) const { return (int64_t)H_[h].pend.size(); }
    const CiBatchStats &stats(int h) const { return H_[h].stats; }
    // the decisions of half h's last round (indep[t], df[t] of test t), in order per edge
    void Resolve(int h, const uint8_t *indep, const int32_t *df);
    // removed / d / sep / counted of the range (launched is the caller's: it knows what it ran)
    void Finish(LevelOut &out);

  private:
    // one edge's search state: the current side's candidate list is adj(a) \ {b}, read in place
    // (element i = base[i + (i >= skip)]), the next combination as positions into it
    struct EdgeState {
        int x, y;
        int side = 0;               // 0: adj(x)\{y}, 1: adj(y)\{x}, 2: exhausted
        const int *base = nullptr;  // adj(a), sorted
        int m = 0;                  // |adj(a) \ {b}|
        int skip = 0;               // position of b in adj(a) (m + 1 if absent)
        int ch[kMaxD];              // next combination (positions in the candidate list)
        bool has_next = false;
        int64_t pos_in_side = 0;    // index of the next combination within the side
        bool resolved = false, removed = false;
        int A(int i) const { return base[i + (i >= skip)]; }
    };
    struct Pending {  // one generated test
        int edge;
        int side;
        int64_t group_end;  // first position after this test's group (within the side)
    };
    struct Half {
        size_t e0, e1;
        int64_t chunk;
        std::vector<int32_t> items;
        std::vector<Pending> pend;
        CiBatchStats stats;
    };
    void StartSide(EdgeState &e) const;
    void Advance(EdgeState &e) const;
    void NextSide(EdgeState &e) const;
    void GenerateSlices(Half &hf);
    void GenerateGroups(Half &hf);

    const Skeleton &sk_;
    const int d_, group_size_;
    const int32_t *dims_;
    const int64_t growth_;
    const bool general_;
    bool full_ = false;  // one round takes every candidate set of the level (all_ of them)
    int64_t all_ = 0;
    int nh_ = 1;
    std::vector<EdgeState> st_;
    Half H_[2];
    std::vector<int> sep_;
    int64_t counted_ = 0;
};

}  // namespace fbn

#endif
