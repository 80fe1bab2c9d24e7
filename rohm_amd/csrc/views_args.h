// What the entry points that take V views of [N, J] keypoints (multiview.hip, rig.hip, sync.hip, fit_views.hip) share on the host
// side: the limits and the refusals of a bad shape.  Every refusal names the entry point; the headers state the texts.
#pragma once
#include "common.h"

namespace rohm {

constexpr int kViewsMax = 16;
constexpr long long kViewsMaxPoints = 1ll << 29;     // N * J

// V in [v_min, kViewsMax], N >= n_min, J >= 1, N * J within the limit: refused in this order
inline int views_check_shape(const char* who, int V, int v_min, int N, int n_min, int J) {
    ROHM_ARG_CHECK(V >= v_min && V <= kViewsMax, "%s: V must be in [%d, %d], got %d", who, v_min, kViewsMax, V);
    ROHM_ARG_CHECK(N >= n_min, "%s: N must be >= %d, got %d", who, n_min, N);
    ROHM_ARG_CHECK(J >= 1, "%s: J must be >= 1, got %d", who, J);
    ROHM_ARG_CHECK((long long)N * J <= kViewsMaxPoints, "%s: N * J must not exceed %lld, got %lld", who, kViewsMaxPoints, (long long)N * J);
    return ROHM_OK;
}

inline int views_check_conf(const char* who, double conf_min) {
    ROHM_ARG_CHECK(isfinite(conf_min), "%s: conf_min must be finite", who);
    return ROHM_OK;
}

// the arguments of a *_ws_bytes function: P = N * J points of V >= 2 views
inline int views_check_ws(const char* who, int V, long long P) {
    ROHM_ARG_CHECK(V >= 2 && V <= kViewsMax, "%s: V must be in [2, %d], got %d", who, kViewsMax, V);
    ROHM_ARG_CHECK(P >= 1 && P <= kViewsMaxPoints, "%s: P must be in [1, %lld], got %lld", who, kViewsMaxPoints, P);
    return ROHM_OK;
}

}  // namespace rohm
