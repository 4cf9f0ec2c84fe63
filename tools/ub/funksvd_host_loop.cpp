// funksvd_host_loop.cpp -- the yardstick of tools/funksvd_time.py: the FunkSVD epoch as a plain
// sequential host loop over the shuffled samples (the arithmetic of src/accel/funksvd.rs:98-124,
// float64, nothing contracted), compiled at -O2 into a shared object the tool loads:
//     c++ -O2 -ffp-contract=off -shared -fPIC -o tools/ub/funksvd_host_loop.so \
//         tools/ub/funksvd_host_loop.cpp
#include <stdint.h>

extern "C" double funksvd_host_epochs(const int32_t *users, const int32_t *items,
                                      const float *ratings, const float *est, int64_t n,
                                      float *ucol, float *icol, int32_t epochs, double lr,
                                      double reg, double trail, double rmin, double rmax)
{
    double sse = 0.0;
    for (int32_t e = 0; e < epochs; ++e) {
        sse = 0.0;
        for (int64_t s = 0; s < n; ++s) {
            float *ufr = ucol + users[s];
            float *ifr = icol + items[s];
            const double ufv = *ufr, ifv = *ifr;
            double pred = (double)est[s] + ufv * ifv + trail;
            if (pred < rmin) pred = rmin;
            if (pred > rmax) pred = rmax;
            const double error = (double)ratings[s] - pred;
            sse += error * error;
            const double ufd = (error * ifv - reg * ufv) * lr;
            const double ifd = (error * ufv - reg * ifv) * lr;
            *ufr = (float)(ufv + ufd);
            *ifr = (float)(ifv + ifd);
        }
    }
    return sse;
}
