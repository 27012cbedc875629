// qcart_host.hpp — host-side pieces the device-handle translation units (qcart_actor.hip, qcart_learner.hip,
// qcart_replay.hip) share: the device guard, the error paths, the create-time checks, and for the DQN handles
// the fragment layout and the layer validation. Internal: not part of the C ABI (include/qcart.h).
#pragma once
#include <hip/hip_runtime.h>

#include <mutex>
#include <string>

#include "../../include/qcart.h"
#include "qcart_mfma.hpp"

namespace qcart {
namespace host {

// makes `d` the current device for a scope
struct Dev {
    int prev = -1;
    explicit Dev(int d) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != d) (void)hipSetDevice(d);
    }
    ~Dev() {
        int cur = -1;
        if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
    }
};

// a HIP failure on a live handle: "<what>: <hipGetErrorString>" into its err string
inline int hip_fail(std::string& err, hipError_t e, const char* what) {
    err = std::string(what) + ": " + hipGetErrorString(e);
    return QC_EHIP;
}

// the error text of a failed qc_*_create (no handle exists yet): one per handle type
class CreateError {
public:
    int fail(const std::string& m, int rc) {
        std::lock_guard<std::mutex> lk(mu_);
        msg_ = m;
        return rc;
    }
    const char* text() {
        std::lock_guard<std::mutex> lk(mu_);
        return msg_.c_str();
    }

private:
    std::mutex mu_;
    std::string msg_;
};

// QC_OK, or the create-time error for a device index that cannot be used; who: "the actor", "libqcart", ...
inline int check_device(int device, CreateError& g, const char* who) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return g.fail(std::string("no HIP device available (") + who + " has no CPU fallback)", QC_EHIP);
    if (device < 0 || device >= ndev) return g.fail("device index out of range", QC_EINVAL);
    return QC_OK;
}

// fragment buffer of n layers [O][Kpad]: per layer the weight fragments u, the sigma_w fragments s (layers that
// may be noisy), the bias ub padded to tiles * 32 and sigma_b likewise; returns the floats taken from `off` on
template <class T>
T frag_layout(int n, const int* O, const int* Kpad, const bool* noisy, T* u, T* s, T* ub, T* sb, T off = 0) {
    for (int l = 0; l < n; ++l) {
        const T fr = (T)mfma::tiles(O[l]) * mfma::ksteps(Kpad[l]) * 64, bp = (T)mfma::tiles(O[l]) * 32;
        u[l] = off; off += fr;
        s[l] = off; off += noisy[l] ? fr : 0;
        ub[l] = off; off += bp;
        sb[l] = off; off += noisy[l] ? bp : 0;
    }
    return off;
}

// which of weight_norm / sigma_w / sigma_b a layer carries, as a 3-bit state, and the sets of states a rule bans
constexpr unsigned kWn = 1, kSw = 2, kSb = 4;
template <class F>
constexpr unsigned states_where(F f) {
    unsigned m = 0;
    for (unsigned s = 0; s < 8; ++s)
        if (f((s & kWn) != 0, (s & kSw) != 0, (s & kSb) != 0)) m |= 1u << s;
    return m;
}
struct LayerRule {
    unsigned layers;   // bit l: the rule applies to layer l
    unsigned banned;   // states_where(...)
    const char* text;
};

// every layer needs weight and bias; then the first rule a layer breaks (layer by layer, rules in order) is the error
inline int validate_layers(const qc_dqn_layer* layers, int n, const LayerRule* rules, int n_rules, std::string& err) {
    for (int l = 0; l < n; ++l) {
        const qc_dqn_layer& L = layers[l];
        if (!L.weight || !L.bias) {
            err = "layer " + std::to_string(l) + ": weight and bias are required";
            return QC_EINVAL;
        }
        const unsigned st = (L.weight_norm ? kWn : 0) | (L.sigma_w ? kSw : 0) | (L.sigma_b ? kSb : 0);
        for (int r = 0; r < n_rules; ++r)
            if ((rules[r].layers >> l & 1) && (rules[r].banned >> st & 1)) {
                err = rules[r].text;
                return QC_EINVAL;
            }
    }
    return QC_OK;
}
constexpr unsigned kSigmaApart = states_where([](bool, bool sw, bool sb) { return sw != sb; });
constexpr const char* kSigmaApartText = "sigma_w and sigma_b go together";

}  // namespace host
}  // namespace qcart
