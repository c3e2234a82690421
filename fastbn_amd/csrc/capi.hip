// capi.hip -- the extern "C" boundary (include/fastbn.h), the entries that own no device state: errors,
// version, device count, networks, datasets, evidence files.  The junction tree is in capi_jt.hip, the
// CI tests and parameter learning in capi_ci.hip, PC-stable in capi_pc.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <memory>
#include <new>

#include "fbn_internal.h"

using fbn::SetError;

extern "C" {

const char *fbn_last_error(void) { return fbn::LastError(); }

int fbn_version(int *major, int *minor) {
    if (major) *major = 0;
    if (minor) *minor = 1;
    return FBN_OK;
}

int fbn_device_count(int *n) {
    if (!n) return SetError(FBN_ERR_ARG, "null pointer");
    int c = 0;
    if (hipGetDeviceCount(&c) != hipSuccess) c = 0;
    *n = c;
    return FBN_OK;
}

// ------------------------------------------------------------------ networks & data
int fbn_network_load_xmlbif(const char *path, fbn_network **out) {
    if (!path || !out) return SetError(FBN_ERR_ARG, "null pointer");
    auto h = std::unique_ptr<fbn_network>(new (std::nothrow) fbn_network());
    if (!h) return SetError(FBN_ERR_NOMEM, "out of memory");
    int rc = fbn::LoadXmlbif(path, h->net);
    if (rc) return rc;
    *out = h.release();
    return FBN_OK;
}
int fbn_network_create(int nvars, const int32_t *dims, const int32_t *parent_off, const int32_t *parents,
                       const int64_t *counts, const char *const *names, fbn_network **out) {
    if (!out) return SetError(FBN_ERR_ARG, "null pointer");
    auto h = std::unique_ptr<fbn_network>(new (std::nothrow) fbn_network());
    if (!h) return SetError(FBN_ERR_NOMEM, "out of memory");
    int rc = fbn::BuildNetwork(nvars, dims, parent_off, parents, counts, names, h->net);
    if (rc) return rc;
    *out = h.release();
    return FBN_OK;
}
int fbn_network_create_cpt(int nvars, const int32_t *dims, const int32_t *parent_off, const int32_t *parents,
                           const double *cpt, const char *const *names, fbn_network **out) {
    if (!out) return SetError(FBN_ERR_ARG, "null pointer");
    auto h = std::unique_ptr<fbn_network>(new (std::nothrow) fbn_network());
    if (!h) return SetError(FBN_ERR_NOMEM, "out of memory");
    int rc = fbn::BuildNetworkCpt(nvars, dims, parent_off, parents, cpt, names, h->net);
    if (rc) return rc;
    *out = h.release();
    return FBN_OK;
}
int fbn_network_node_probs(const fbn_network *net, int node, int32_t *parents, double *probs, int *nparents,
                           int64_t *nprobs) {
    if (!net) return SetError(FBN_ERR_ARG, "null pointer");
    return fbn::NodeProbs(net->net, node, parents, probs, nparents, nprobs);
}
int fbn_network_node_counts(const fbn_network *net, int node, int32_t *parents, int64_t *counts, int *nparents,
                            int64_t *ncounts) {
    if (!net) return SetError(FBN_ERR_ARG, "null pointer");
    return fbn::NodeCounts(net->net, node, parents, counts, nparents, ncounts);
}
int fbn_network_num_nodes(const fbn_network *net, int *n) {
    if (!net || !n) return SetError(FBN_ERR_ARG, "null pointer");
    *n = net->net.n();
    return FBN_OK;
}
int fbn_network_dims(const fbn_network *net, int32_t *dims) {
    if (!net || !dims) return SetError(FBN_ERR_ARG, "null pointer");
    for (int i = 0; i < net->net.n(); ++i) dims[i] = net->net.dom[i];
    return FBN_OK;
}
int fbn_network_name(const fbn_network *net, int node, char *buf, int cap) {
    if (!net || !buf || cap <= 0 || node < 0 || node >= net->net.n()) return SetError(FBN_ERR_ARG, "bad argument");
    snprintf(buf, cap, "%s", net->net.names[node].c_str());
    return FBN_OK;
}
int fbn_network_destroy(fbn_network *net) {
    delete net;
    return FBN_OK;
}

int fbn_evidence_load_libsvm(const char *path, int num_nodes, int8_t *evidence, int32_t *labels, int64_t cap,
                             int64_t *ncases) {
    if (!path || num_nodes <= 0) return SetError(FBN_ERR_ARG, "bad argument");
    // streaming parse straight into the caller's rows (no intermediate copy)
    return fbn::LoadLibsvm(path, num_nodes, evidence && cap > 0 ? evidence : nullptr, labels, cap, ncases);
}

int fbn_dataset_load_csv(const char *path, fbn_dataset **out) {
    if (!path || !out) return SetError(FBN_ERR_ARG, "null pointer");
    auto h = std::unique_ptr<fbn_dataset>(new (std::nothrow) fbn_dataset());
    if (!h) return SetError(FBN_ERR_NOMEM, "out of memory");
    int rc = fbn::LoadCsv(path, h->ds);
    if (rc) return rc;
    *out = h.release();
    return FBN_OK;
}
int fbn_dataset_shape(const fbn_dataset *ds, int *nvars, int64_t *nsamples) {
    if (!ds) return SetError(FBN_ERR_ARG, "null pointer");
    if (nvars) *nvars = ds->ds.nvars;
    if (nsamples) *nsamples = ds->ds.nsamples;
    return FBN_OK;
}
int fbn_dataset_dims(const fbn_dataset *ds, int32_t *dims) {
    if (!ds || !dims) return SetError(FBN_ERR_ARG, "null pointer");
    std::copy(ds->ds.dims.begin(), ds->ds.dims.end(), dims);
    return FBN_OK;
}
int fbn_dataset_columns(const fbn_dataset *ds, uint8_t *cols) {
    if (!ds || !cols) return SetError(FBN_ERR_ARG, "null pointer");
    std::copy(ds->ds.cols.begin(), ds->ds.cols.end(), cols);
    return FBN_OK;
}
int fbn_dataset_var_name(const fbn_dataset *ds, int v, char *buf, int cap) {
    if (!ds || !buf || cap <= 0 || v < 0 || v >= ds->ds.nvars) return SetError(FBN_ERR_ARG, "bad argument");
    snprintf(buf, cap, "%s", ds->ds.names[v].c_str());
    return FBN_OK;
}
int fbn_dataset_destroy(fbn_dataset *ds) {
    delete ds;
    return FBN_OK;
}

}  // extern "C"
