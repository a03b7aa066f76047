/* Piecewise-linear look-up of a tabulated E/N coefficient: value and d/dE, for host and device.
 *
 * Knots x[0..n) strictly increasing (V/m), n >= 1 -- the creator checks that; nothing here does.
 *   value       np.interp's: y[0] for E <= x[0], y[n-1] for E >= x[n-1], else slope_j (E - x[j]) + y[j] with
 *               x[j] <= E < x[j+1] and slope_j = (y[j+1] - y[j]) / (x[j+1] - x[j])  (the form of gdprep.hip's interp1)
 *   derivative  slope_j for x[0] <= E < x[n-1]; exactly 0 outside and for n == 1
 *   NaN         a NaN argument gives a NaN value and a NaN derivative
 * The segment index lies in [0, max(n - 2, 0)] for ANY argument (NaN, +-inf, 0, negative): the comparisons of the
 * search can only keep it there, and it is clamped besides.  No array entry outside [0, n) is ever read.
 *
 * No HIP include: a host compiler takes this file as it is (tests/test_table_lookup.py compiles it alone). */
#ifndef FEDM_TABLE_LOOKUP_H
#define FEDM_TABLE_LOOKUP_H

#ifdef __HIPCC__
#define FEDM_TABLE_FN __host__ __device__ static inline
#else
#define FEDM_TABLE_FN static inline
#endif

/* j with x[j] <= E < x[j+1] where there is one; 0 or the last segment otherwise */
FEDM_TABLE_FN int fedm_table_segment(const double *x, int n, double E) {
    int lo = 0, hi = n - 1;
    while (hi - lo > 1) {
        const int mid = lo + ((hi - lo) >> 1); /* lo < mid < hi */
        if (x[mid] <= E) lo = mid;             /* false for NaN: lo stays */
        else hi = mid;
    }
    const int last = n >= 2 ? n - 2 : 0;
    return lo < 0 ? 0 : (lo > last ? last : lo);
}

FEDM_TABLE_FN void fedm_table_eval(const double *x, const double *y, int n, double E, double *val, double *der) {
    if (E != E) { /* NaN in, NaN out */
        *val = E;
        *der = E;
        return;
    }
    *der = 0.0;
    if (n < 2 || E <= x[0]) {
        *val = y[0];
        if (n >= 2 && E == x[0]) *der = (y[1] - y[0]) / (x[1] - x[0]);
        return;
    }
    if (E >= x[n - 1]) {
        *val = y[n - 1];
        return;
    }
    const int j = fedm_table_segment(x, n, E);
    const double slope = (y[j + 1] - y[j]) / (x[j + 1] - x[j]);
    *val = slope * (E - x[j]) + y[j];
    *der = slope;
}

#endif /* FEDM_TABLE_LOOKUP_H */
