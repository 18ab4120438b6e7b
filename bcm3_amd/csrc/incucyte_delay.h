// incucyte_delay.h -- the delay parts CVODESolverDelay (src/odecommon/CVODESolverDelay.cpp) adds to
// CVODE, for the one-trajectory-per-wavefront Incucyte kernel (incucyte_kernel.hip):
//   * the history of accepted steps (Simulate, :171-177 and :257-265) in device memory, and
//   * InterpolateHistory (:271-349) on it.
// The Incucyte right-hand side reads component 1 of the delayed state only, so an entry is the pair
// (t, y[1]): 2000 x 16 B per trajectory. Every lane of the wavefront holds the same values and makes
// the same (same-address, same-value) stores, so each lane reads back what it wrote itself.
#pragma once
#include <hip/hip_runtime.h>

#include "bdf_lane.h"

namespace bcm3hip {

struct DelayHistory {
    double2* h;  // [capacity] (t, y1), times strictly increasing
    int n;       // entries stored
    // first and last column in registers: outside the stored range the value is clamped to them,
    // which is every query while t < apoptosis_duration
    double t_first, y_first, t_last, y_last;
    mutable int cur;  // lower index of the last bracketing interval (queries move slowly forward)

    BDF_INL void start(double2* mem, double t, double y1)
    {
        h = mem;
        h[0] = make_double2(t, y1);
        n = 1;
        t_first = t_last = t;
        y_first = y_last = y1;
        cur = 0;
    }
    BDF_INL void push(double t, double y1)
    {
        h[n] = make_double2(t, y1);
        n++;
        t_last = t;
        y_last = y1;
    }
    // InterpolateHistory(t)(1): the first / last column outside the stored range, the stored column
    // on an exact hit, linear interpolation inside the (unique) bracketing interval otherwise. The
    // reference bisects; any search finds the same interval, and the cursor usually moves by 0 or 1.
    BDF_INL double at(double t) const
    {
        if (t <= t_first) return y_first;
        if (t >= t_last) return y_last;
        if (!(t == t)) return y_last;  // (a NaN time: the reference's bisection gives up; never on a finite solve)
        int i = cur;
        i = (i > n - 2) ? n - 2 : i;
        double2 lo = h[i];
        while (i > 0 && lo.x > t) {
            i--;
            lo = h[i];
        }
        double2 hi = h[i + 1];
        while (i < n - 2 && hi.x <= t) {
            i++;
            lo = hi;
            hi = h[i + 1];
        }
        cur = i;
        if (lo.x == t) return lo.y;
        const double a = (t - lo.x) / (hi.x - lo.x);
        return lo.y + a * (hi.y - lo.y);
    }
};

}  // namespace bcm3hip
