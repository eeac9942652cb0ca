// qk_shadow_bound (quake_amd/csrc/qk_shadow_bound.h), the error bound of the fp16 shadow form, on edge values: zeros, subnormals,
// the largest finite floats, infinities, NaN, negative arguments, every d.  What it must do there: return a finite value >= 0, or
// the "no bound" value -1, never NaN or infinity, and grow with every argument.  Built and run by tests/test_shadow_bound.py
// (g++ with the address and undefined-behaviour sanitizers, no GPU).
#include "qk_shadow_bound.h"

#include <cfloat>
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

static int failures = 0;

static void expect(bool ok, const char *what, float a, float b, float c, float d, float got) {
    if (ok) return;
    failures++;
    printf("FAIL %s: qn=%g rho_q=%g rho=%g xmax=%g -> %g\n", what, a, b, c, d, got);
}

int main() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const std::vector<float> vals = {0.0f, FLT_TRUE_MIN, FLT_MIN, 1e-20f, 6.1e-5f, 1e-3f, 1.0f, 15.0f, 65504.0f, 1e6f, 1e18f, 1e19f, FLT_MAX, inf, nan, -0.0f, -1.0f};
    for (int l2 = 0; l2 <= 1; l2++)
        for (int d : {-1, 0, 1, 2, 15, 16, 17, 31, 32, 33, 128, 255, 256, 8192})
            for (float a : vals)
                for (float b : vals)
                    for (float c : vals)
                        for (float e : vals) {
                            const float r = qk_shadow_bound(l2, d, a, b, c, e);
                            const bool bad_arg = d <= 0 || !(a >= 0.f) || !(b >= 0.f) || !(c >= 0.f) || !(e >= 0.f);
                            expect(r == r && std::fabs(r) <= FLT_MAX, "finite", a, b, c, e, r);
                            expect(r == -1.0f || r > 0.0f, "positive or no bound", a, b, c, e, r);
                            if (bad_arg) expect(r == -1.0f, "bad argument refused", a, b, c, e, r);
                            if (a == inf || b == inf || c == inf || e == inf) expect(r == -1.0f, "infinity refused", a, b, c, e, r);
                        }
    // monotone in every argument (a larger norm or error never tightens the bound)
    for (int l2 = 0; l2 <= 1; l2++)
        for (float a : {0.0f, 1e-3f, 1.0f, 15.0f, 6e4f})
            for (float c : {0.0f, 1e-4f, 3e-3f, 1.0f}) {
                const float r0 = qk_shadow_bound(l2, 128, a, 1e-3f, c, 15.0f);
                expect(qk_shadow_bound(l2, 128, a * 2 + 1, 1e-3f, c, 15.0f) >= r0, "monotone in qn", a, 1e-3f, c, 15.0f, r0);
                expect(qk_shadow_bound(l2, 128, a, 2e-3f, c, 15.0f) >= r0, "monotone in rho_q", a, 1e-3f, c, 15.0f, r0);
                expect(qk_shadow_bound(l2, 128, a, 1e-3f, c * 2 + 1e-4f, 15.0f) >= r0, "monotone in rho", a, 1e-3f, c, 15.0f, r0);
                expect(qk_shadow_bound(l2, 128, a, 1e-3f, c, 30.0f) >= r0, "monotone in xmax", a, 1e-3f, c, 15.0f, r0);
                expect(qk_shadow_bound(l2, 256, a, 1e-3f, c, 15.0f) >= r0, "monotone in d", a, 1e-3f, c, 15.0f, r0);
            }
    // exact inputs (integers an fp16 holds): only the fp32 terms are left -- under 1e-4 of (||q|| + ||x||)^2, the scale of the keys
    expect(qk_shadow_bound(1, 128, 200.0f, 0.0f, 0.0f, 200.0f) < 1e-4f * 400.0f * 400.0f, "small for exact inputs", 200.0f, 0.0f, 0.0f, 200.0f,
           qk_shadow_bound(1, 128, 200.0f, 0.0f, 0.0f, 200.0f));
    if (failures) {
        printf("%d failures\n", failures);
        return 1;
    }
    printf("ok\n");
    return 0;
}
