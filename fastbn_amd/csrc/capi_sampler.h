// capi_sampler.h -- the base of the case-sampling handles fbn_sampler (capi_sample.hip), fbn_epis
// (capi_epis.hip) and fbn_ais (capi_ais.hip): the flattened network and its uploaded tables, the
// staging buffers of the host-buffer entries, and the steps every device run and every host-buffer run
// of the three takes.  The device, events and streams are DeviceHandle's (fbn_device.h).  What is
// specific to a sampler stays in its handle.
// Internal to libfastbn.
#ifndef FBN_CAPI_SAMPLER_H
#define FBN_CAPI_SAMPLER_H

#include <hip/hip_runtime.h>

#include <cstring>

#include "fbn_device.h"
#include "fbn_internal.h"
#include "sample_device.h"
#include "sample_model.h"

namespace fbn {

struct SamplerHandle : DeviceHandle {
    SamplerModel M;
    DevBuf nodes, par, prob, cdf, ent;
    DevBuf evid, labels, marg, stats, dv, dm, de, scratch;  // staging of the host-buffer entries; labels-only accumulators

    // device >= 0: check it, upload the tables (the cdf rows only for the handles that read them), create
    // the events; device < 0: a host-only handle
    int AttachTables(int dev, bool with_cdf) {
        if (dev < 0) return FBN_OK;
        int r;
        if ((r = Attach(dev)) || (r = Upload(nodes, M.nodes)) || (r = Upload(par, M.par)) ||
            (r = Upload(prob, M.prob)) || (with_cdf && (r = Upload(cdf, M.cdf))) || (r = Upload(ent, M.ent)))
            return r;
        return evidence.Attach(M.dom);
    }
    int Create(const Network &net, int dev, bool with_cdf) {
        if (int rc = BuildSamplerModel(net, M)) return rc;
        return AttachTables(dev, with_cdf);
    }
    DeviceModel View() const {
        return DeviceModel{nodes.as<SampleNode>(), par.as<int32_t>(), prob.as<double>(), cdf.as<double>(),
                           ent.as<int32_t>(), M.V, M.sum_dom, M.dom[0]};
    }

    // The opening of a device run of ncases cases: the launch limit, the stream's bookkeeping, the evidence
    // check (as fbn_jt_run_device's: on the device, one stream sync) and, for a labels-only run, the
    // accumulator rows in the handle.
    int OpenRun(const int8_t *d_ev, int64_t ncases, double **d_marg, hipStream_t st) {
        if (ncases > 0x7fffffffll) return SetError(FBN_ERR_LIMIT, "%lld cases in one call", (long long)ncases);
        Note(st);
        if (int rc = evidence.Run(d_ev, ncases, st)) return rc;
        if (!*d_marg) {
            if (int rc = scratch.ensure((size_t)ncases * M.sum_dom * 8)) return rc;
            *d_marg = scratch.as<double>();
        }
        return FBN_OK;
    }
    // The common arguments of a run: the seeded stream R (left to the caller for further jumps), the jump
    // from a chunk to the next, the case range and the buffers.
    void FillArgs(SampleCaseArgs &a, PcgStream &R, uint64_t seed, const int8_t *d_ev, int64_t ncases, int64_t S,
                  int64_t case_offset, int32_t *d_labels, double *d_marg, double *d_stats, uint8_t *d_dv, double *d_dm,
                  int32_t *d_de) const {
        PcgStreamInit(seed, R);
        memcpy(a.jump, R.jump, sizeof a.jump);
        a.M = View();
        a.state = R.state, a.inc = R.inc;
        PcgJump(R, (uint64_t)63 * (uint64_t)M.V, &a.jm, &a.jc);
        a.ev = d_ev;
        a.ncases = ncases, a.S = S, a.case0 = case_offset;
        a.labels = d_labels, a.marg = d_marg, a.stats = d_stats;
        a.dv = d_dv, a.dm = d_dm, a.de = d_de;
    }

    // A run on host buffers (device >= 0): stage the evidence, run, copy back.  stats_doubles: the width of
    // a stats row; draws: samples per case in the debug arrays (values: all three or none).  extra: one more
    // debug array that comes with values, extra_bytes of *extra after the run into extra_host, or NULL.
    // run(d_ev, d_labels, d_marg, d_stats, d_dv, d_dm, d_de) is the handle's device run on the null stream.
    template <class Run>
    int HostBuffers(const int8_t *evidence, int64_t ncases, int stats_doubles, int64_t draws, int32_t *h_labels,
                    double *h_marg, double *h_stats, uint8_t *values, double *mant, int32_t *expo, DevBuf *extra,
                    size_t extra_bytes, void *extra_host, Run run) {
        FBN_HIP(hipSetDevice(device));
        const size_t V = (size_t)M.V, n = (size_t)ncases, total = n * (size_t)draws;
        const size_t mbytes = n * (size_t)M.sum_dom * 8, sbytes = n * (size_t)stats_doubles * 8;
        int rc;
        if ((rc = evid.ensure(n * V)) || (rc = labels.ensure(n * 4)) || (rc = marg.ensure(mbytes)) ||
            (rc = stats.ensure(sbytes)))
            return rc;
        if (values && ((rc = dv.ensure(total * V)) || (rc = dm.ensure(total * 8)) || (rc = de.ensure(total * 4)) ||
                       (extra && (rc = extra->ensure(extra_bytes)))))
            return rc;
        FBN_HIP(hipMemcpy(evid.p, evidence, n * V, hipMemcpyHostToDevice));
        rc = run(evid.as<int8_t>(), labels.as<int32_t>(), marg.as<double>(), stats.as<double>(),
                 values ? dv.as<uint8_t>() : nullptr, values ? dm.as<double>() : nullptr,
                 values ? de.as<int32_t>() : nullptr);
        if (rc) return rc;
        FBN_HIP(hipMemcpy(h_labels, labels.p, n * 4, hipMemcpyDeviceToHost));
        if (h_marg) FBN_HIP(hipMemcpy(h_marg, marg.p, mbytes, hipMemcpyDeviceToHost));
        if (h_stats) FBN_HIP(hipMemcpy(h_stats, stats.p, sbytes, hipMemcpyDeviceToHost));
        if (values) {
            FBN_HIP(hipMemcpy(values, dv.p, total * V, hipMemcpyDeviceToHost));
            FBN_HIP(hipMemcpy(mant, dm.p, total * 8, hipMemcpyDeviceToHost));
            FBN_HIP(hipMemcpy(expo, de.p, total * 4, hipMemcpyDeviceToHost));
            if (extra) FBN_HIP(hipMemcpy(extra_host, extra->p, extra_bytes, hipMemcpyDeviceToHost));
        }
        return FBN_OK;
    }
};

}  // namespace fbn

#endif
