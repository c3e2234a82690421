// param_learn.cpp -- host side of parameter learning: family sizing / validation and the PDAG -> DAG
// extension.  No device and no other part of the library: it compiles on its own (with a main that
// supplies fbn::SetError) for host-side sanitizer runs.
//
// ParamFamilySizes: the table shapes of every node of a graph given as CSR parent lists -- what
// DiscreteNode::InitializeCPT enumerates per node (src/DiscreteNode.cpp:114-130: every value of the
// node x every configuration of its parents) -- as per-node offsets into one array, node v's table
// being counts[value][parent configuration] (fbn_network_create's layout).  Cap: a family, and the
// sum over the families, holds at most FBN_PARAM_MAX_CELLS = 2^26 cells; every product and sum is
// checked against the cap BEFORE it is formed (the running value never exceeds 2^26 * 256 = 2^34),
// so the product of up to nvars state counts cannot wrap.
//
// PdagToDag: a consistent DAG extension of a partially directed graph (Dor & Tarsi, "A simple
// algorithm to construct a consistent extension of a partially oriented graph", 1992).  The
// reference has no counterpart: StructLearnCompData stops at the CPDAG (src/PCStable.cpp:576-843)
// and ParameterLearning::LearnParamsKnowStructCompData (src/ParameterLearning.cpp:11-64) is only
// given DAGs read from a network file.
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "fbn_internal.h"

namespace fbn {

int ParamFamilySizes(int nvars, const int32_t *dims, const int32_t *parent_off, const int32_t *parents,
                     int64_t *family_off, int64_t *ncounts) {
    if (nvars < 1 || !dims || !parent_off) return SetError(FBN_ERR_ARG, "family sizes: bad arguments");
    if (parent_off[0] != 0) return SetError(FBN_ERR_ARG, "family sizes: parent_off[0] = %d, not 0", parent_off[0]);
    for (int v = 0; v < nvars; ++v) {
        if (dims[v] < 1 || dims[v] > 256) return SetError(FBN_ERR_ARG, "dims[%d] = %d out of 1..256", v, dims[v]);
        if (parent_off[v + 1] < parent_off[v]) return SetError(FBN_ERR_ARG, "node %d: parent offsets decrease", v);
    }
    if (parent_off[nvars] > 0 && !parents) return SetError(FBN_ERR_ARG, "family sizes: parents missing");
    const int64_t cap = FBN_PARAM_MAX_CELLS;
    std::vector<int32_t> seen(nvars, -1);  // seen[q] = v: q already listed as a parent of v
    int64_t total = 0;
    for (int v = 0; v < nvars; ++v) {
        if (family_off) family_off[v] = total;
        int64_t cells = dims[v];
        for (int32_t k = parent_off[v]; k < parent_off[v + 1]; ++k) {
            const int32_t q = parents[k];
            if (q < 0 || q >= nvars) return SetError(FBN_ERR_ARG, "node %d: parent %d out of range", v, q);
            if (q == v) return SetError(FBN_ERR_ARG, "node %d: is its own parent", v);
            if (seen[q] == v) return SetError(FBN_ERR_ARG, "node %d: repeated parent %d", v, q);
            seen[q] = v;
        }
        // validation of the whole list first, then the product: cells <= cap before each multiply,
        // the factor <= 256, so the product stays below 2^34
        for (int32_t k = parent_off[v]; k < parent_off[v + 1]; ++k) {
            cells *= dims[parents[k]];
            if (cells > cap)
                return SetError(FBN_ERR_LIMIT, "node %d: its family has more than %lld cells (the cap)", v, (long long)cap);
        }
        total += cells;  // both <= cap
        if (total > cap)
            return SetError(FBN_ERR_LIMIT, "families up to node %d hold more than %lld cells (the cap)", v, (long long)cap);
    }
    if (family_off) family_off[nvars] = total;
    if (ncounts) *ncounts = total;
    return FBN_OK;
}

int PdagToDag(int nvars, const int32_t *triples, int n, int32_t *parent_off, int32_t *parents) {
    if (nvars < 1 || n < 0 || (!triples && n > 0) || !parent_off || (!parents && n > 0))
        return SetError(FBN_ERR_ARG, "pdag_to_dag: bad arguments");
    // adjacency as sorted neighbour lists: arcs out / in, undirected
    std::vector<std::vector<int>> out(nvars), in(nvars), und(nvars);
    {
        std::vector<std::pair<int, int>> keys;  // unordered pairs, for the duplicate check
        keys.reserve(n);
        for (int e = 0; e < n; ++e) {
            const int a = triples[3 * e], b = triples[3 * e + 1], t = triples[3 * e + 2];
            if (a < 0 || a >= nvars || b < 0 || b >= nvars) return SetError(FBN_ERR_ARG, "edge %d: node out of range", e);
            if (a == b) return SetError(FBN_ERR_ARG, "edge %d: self loop at node %d", e, a);
            if (t != 0 && t != 1) return SetError(FBN_ERR_ARG, "edge %d: type %d is neither 0 nor 1", e, t);
            keys.emplace_back(std::min(a, b), std::max(a, b));
            if (t) out[a].push_back(b), in[b].push_back(a);
            else und[a].push_back(b), und[b].push_back(a);
        }
        std::sort(keys.begin(), keys.end());
        for (size_t i = 1; i < keys.size(); ++i)
            if (keys[i] == keys[i - 1])
                return SetError(FBN_ERR_ARG, "nodes %d and %d are joined by more than one edge (duplicate or contradictory)",
                                keys[i].first, keys[i].second);
    }
    // adjacency test by sorted lists (a dense matrix would be nvars^2 bytes)
    std::vector<std::vector<int>> nb(nvars);
    for (int v = 0; v < nvars; ++v) {
        nb[v] = out[v];
        nb[v].insert(nb[v].end(), in[v].begin(), in[v].end());
        nb[v].insert(nb[v].end(), und[v].begin(), und[v].end());
        std::sort(nb[v].begin(), nb[v].end());
    }
    auto adjacent = [&](int a, int b) { return std::binary_search(nb[a].begin(), nb[a].end(), b); };
    std::vector<char> alive(nvars, 1);
    std::vector<std::vector<int>> par(nvars);
    for (int v = 0; v < nvars; ++v) par[v] = in[v];
    for (int left = nvars; left > 0; --left) {
        int pick = -1;
        for (int x = 0; x < nvars && pick < 0; ++x) {
            if (!alive[x]) continue;
            bool ok = true;
            for (int y : out[x])
                if (alive[y]) {
                    ok = false;  // x has an arc to a remaining node: not a sink
                    break;
                }
            // every remaining undirected neighbour y adjacent to all of x's other remaining neighbours
            for (size_t i = 0; ok && i < und[x].size(); ++i) {
                const int y = und[x][i];
                if (!alive[y]) continue;
                for (int z : nb[x])
                    if (alive[z] && z != y && !adjacent(y, z)) {
                        ok = false;
                        break;
                    }
            }
            if (ok) pick = x;
        }
        if (pick < 0) {
            std::string rest;
            int shown = 0;
            for (int v = 0; v < nvars; ++v)
                if (alive[v]) {
                    if (shown == 16) {
                        rest += " ...";
                        break;
                    }
                    rest += (shown++ ? " " : "") + std::to_string(v);
                }
            return SetError(FBN_ERR_ARG, "no consistent DAG extension (or a directed cycle): %d nodes remain: %s", left,
                            rest.c_str());
        }
        for (int y : und[pick])
            if (alive[y]) par[pick].push_back(y);  // y - pick becomes y -> pick
        alive[pick] = 0;
    }
    int32_t off = 0;
    for (int v = 0; v < nvars; ++v) {
        std::sort(par[v].begin(), par[v].end());
        parent_off[v] = off;
        for (int q : par[v]) parents[off++] = q;
    }
    parent_off[nvars] = off;
    return FBN_OK;
}

}  // namespace fbn
