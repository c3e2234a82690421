// pc_search.cpp -- the combinatorics of one PC-stable level (pc_search.h): edge state, the split
// into halves, chunked generation and in-order resolution.  No device, no knobs.
#include "pc_search.h"

namespace fbn {

namespace {
// a single-round level split in two: the first half takes this share of the candidate sets
constexpr double kFirstHalfShare = 0.20;
}  // namespace

void LevelSearch::StartSide(EdgeState &e) const {
    while (e.side < 2) {
        const int a = e.side ? e.y : e.x, b = e.side ? e.x : e.y;
        const std::vector<int> &L = sk_.adj[a];
        const int pos = (int)(std::lower_bound(L.begin(), L.end(), b) - L.begin());
        const bool has_b = pos < (int)L.size() && L[pos] == b;
        e.base = L.data();
        e.m = (int)L.size() - (has_b ? 1 : 0);
        e.skip = has_b ? pos : (int)L.size() + 1;
        if (e.m >= d_) {
            for (int i = 0; i < d_; ++i) e.ch[i] = i;
            e.has_next = true;
            e.pos_in_side = 0;
            return;
        }
        ++e.side;
    }
    e.has_next = false;
}

void LevelSearch::Advance(EdgeState &e) const {  // ChoiceGenerator::Next (src/ChoiceGenerator.cpp:55-85)
    const int m = e.m, d = d_;
    int i = d - 1;
    while (i >= 0 && e.ch[i] == m - d + i) --i;
    if (i < 0) {
        e.has_next = false;
        return;
    }
    ++e.ch[i];
    for (int k = i + 1; k < d; ++k) e.ch[k] = e.ch[k - 1] + 1;
    ++e.pos_in_side;
}

void LevelSearch::NextSide(EdgeState &e) const {  // side exhausted: the next side starts fresh
    if (e.side == 0) {
        e.side = 1;
        StartSide(e);
    } else {
        e.side = 2;
        e.has_next = false;
    }
}

LevelSearch::LevelSearch(const Skeleton &sk, size_t e_begin, size_t e_end, int d, int group_size, const int32_t *dims,
                         const SearchSchedule &sch)
    : sk_(sk), d_(d), group_size_(group_size), dims_(dims), growth_(std::max<int64_t>(2, sch.growth)),
      general_(sch.general), st_(e_end - e_begin), sep_((e_end - e_begin) * (size_t)d, -1) {
    const size_t E = e_end - e_begin;
    int64_t open_edges = 0;
    for (size_t e = 0; e < E; ++e) {
        st_[e].x = sk.edges[e_begin + e].first;
        st_[e].y = sk.edges[e_begin + e].second;
        StartSide(st_[e]);
        if (!st_[e].has_next) st_[e].resolved = true;  // both sides too small: kept
        open_edges += !st_[e].resolved;
    }
    // first round: enough tests to fill the device (~8k) without speculating deep into edges that
    // usually resolve early; later rounds grow per round
    int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(32, sch.round0 / std::max<int64_t>(1, open_edges)));
    // small levels: every candidate set of every edge in one round (one host round trip per level;
    // the extra speculative tests cost less than the round trips they save)
    for (size_t e = 0; e < E && all_ <= sch.full_spec; ++e)
        if (!st_[e].resolved) all_ += sk.EdgeCost(e_begin + e, d);
    if (all_ <= sch.full_spec) chunk = all_, full_ = true;
    // (a single-round level of many candidate sets -- config-5 level 2, 8.7k -- also splits in two:
    // the second half is generated on the host while the first half's batch runs)
    nh_ = E < 2 ? 1 : full_ ? (chunk >= sch.split_full ? 2 : 1) : (open_edges < sch.pipeline_edges ? 1 : 2);
    for (int h = 0; h < nh_; ++h) H_[h].e0 = E * h / nh_, H_[h].e1 = E * (h + 1) / nh_, H_[h].chunk = chunk;
    if (nh_ == 2) {  // cut where the candidate-set counts of the open edges reach a fraction (the
                     // first half's generation is on the critical path, the second's is not)
        std::vector<double> cost(E, 0.0);
        double tot = 0.0;
        for (size_t e = 0; e < E; ++e)
            if (!st_[e].resolved) tot += cost[e] = (double)sk.EdgeCost(e_begin + e, d);
        double acc = 0.0;
        size_t cut = 0;
        // (config 5 level 2, driver median: 50 % 3.55 ms, 25 % 3.51, 15 % 3.51, 10 % 3.49)
        while (cut < E && acc + cost[cut] <= tot * kFirstHalfShare) acc += cost[cut++];
        H_[0].e1 = H_[1].e0 = std::max<size_t>(1, std::min(cut, E - 1));
    }
}

bool LevelSearch::Generate(int h) {
    Half &hf = H_[h];
    hf.items.clear();
    hf.pend.clear();
    hf.stats = CiBatchStats{0, 0};
    if (d_ == 1 && group_size_ == 1 && !general_) GenerateSlices(hf);
    else GenerateGroups(hf);
    hf.chunk = std::min<int64_t>(hf.chunk * growth_, 1 << 16);
    return !hf.pend.empty();
}

// one conditioning variable, no groups: an edge's next chunk is a contiguous slice of its candidate
// list (with full speculation: both sides whole) -- written into arrays sized up front, without
// per-test bookkeeping (the same tests and state transitions as GenerateGroups)
void LevelSearch::GenerateSlices(Half &hf) {
    const auto &adj = sk_.adj;
    size_t cap = 0;
    for (size_t e = hf.e0; e < hf.e1; ++e) {
        const EdgeState &s = st_[e];
        if (!s.resolved && s.has_next)
            cap += full_ ? adj[s.x].size() + adj[s.y].size() : (size_t)std::min<int64_t>(hf.chunk, s.m - s.ch[0]);
    }
    hf.items.resize(3 * cap);
    hf.pend.resize(cap);
    int32_t *it = hf.items.data();
    Pending *pp = hf.pend.data();
    int64_t rows = 0;
    int mx = 0;
    for (size_t e = hf.e0; e < hf.e1; ++e) {
        EdgeState &s = st_[e];
        if (s.resolved) continue;
        const int dx = dims_[s.x], dy = dims_[s.y];
        while (s.has_next) {
            const int cnt = (int)std::min<int64_t>(hf.chunk, s.m - s.ch[0]);
            mx = std::max(mx, std::max(dx, dy));
            for (int i = 0; i < cnt; ++i) {
                const int z = s.A(s.ch[0] + i);
                it[0] = s.x, it[1] = s.y, it[2] = z, it += 3;
                rows += dx + dy + dims_[z], mx = std::max(mx, dims_[z]);
                *pp++ = Pending{(int)e, s.side, s.pos_in_side + i + 1};
            }
            if (s.ch[0] + cnt == s.m) {
                NextSide(s);
                if (full_ && s.side == 1) continue;  // one round takes every candidate set
            } else {
                s.ch[0] += cnt;
                s.pos_in_side += cnt;
            }
            break;
        }
    }
    const size_t total = (size_t)(pp - hf.pend.data());
    hf.items.resize(3 * total);
    hf.pend.resize(total);
    hf.stats = CiBatchStats{mx, rows};
}

void LevelSearch::GenerateGroups(Half &hf) {
    const int d = d_, group_size = group_size_;
    if (full_) {  // one round takes all candidate sets of the level
        hf.items.reserve((size_t)all_ * (2 + d));
        hf.pend.reserve((size_t)all_);
    }
    for (size_t e = hf.e0; e < hf.e1; ++e) {
        EdgeState &s = st_[e];
        if (s.resolved) continue;
        // next chunk: whole groups only, never across a side boundary
        int64_t want = ((hf.chunk + group_size - 1) / group_size) * group_size;
        while (want > 0 && s.has_next) {
            const int64_t gstart = (s.pos_in_side / group_size) * group_size;
            hf.pend.push_back(Pending{(int)e, s.side, gstart + group_size});
            hf.items.push_back(s.x);
            hf.items.push_back(s.y);
            int r = dims_[s.x] + dims_[s.y], mx = std::max(dims_[s.x], dims_[s.y]);
            for (int i = 0; i < d; ++i) {
                const int z = s.A(s.ch[i]);
                hf.items.push_back(z);
                r += dims_[z], mx = std::max(mx, dims_[z]);
            }
            hf.stats.dim_rows += r, hf.stats.maxdim = std::max(hf.stats.maxdim, mx);
            --want;
            Advance(s);
            if (!s.has_next) {  // (the next side's groups restart at 0)
                NextSide(s);
                // keep groups aligned: a partial chunk ends at the side boundary (not needed when the
                // round takes every candidate set: no group is ever split)
                if (!full_) break;
            }
        }
    }
}

void LevelSearch::Resolve(int h, const uint8_t *indep, const int32_t *df) {
    const Half &hf = H_[h];
    const auto &pend = hf.pend;
    const int d = d_;
    size_t i = 0;
    while (i < pend.size()) {
        const int e = pend[i].edge;
        size_t j = i;
        while (j < pend.size() && pend[j].edge == e) ++j;  // tests of this edge: [i, j)
        EdgeState &s = st_[e];
        size_t k = i;
        while (k < j && !s.removed) {
            // one group: tests with the same side and group_end
            size_t g = k;
            while (g < j && pend[g].side == pend[k].side && pend[g].group_end == pend[k].group_end) ++g;
            const int gsz = (int)(g - k);
            counted_ += gsz;
            for (size_t t = k; t < g; ++t) {
                bool ind = indep[t] != 0;
                if (gsz > 1 && df[t] == 0) ind = false;  // group quirk (see pc_driver.cpp's header)
                if (ind) {
                    s.removed = true;
                    s.resolved = true;
                    int *z = sep_.data() + (size_t)e * d;
                    std::copy(hf.items.begin() + (2 + d) * t + 2, hf.items.begin() + (2 + d) * (t + 1), z);
                    std::sort(z, z + d);
                    break;
                }
            }
            k = g;
        }
        if (!s.removed && !s.has_next) s.resolved = true;  // exhausted: dependent, kept
        i = j;
    }
}

void LevelSearch::Finish(LevelOut &out) {
    out.removed.assign(st_.size(), 0);
    for (size_t e = 0; e < st_.size(); ++e)
        if (st_[e].removed) out.removed[e] = 1;
    out.d = d_;
    out.sep.swap(sep_);
    out.counted = counted_;
}

}  // namespace fbn
