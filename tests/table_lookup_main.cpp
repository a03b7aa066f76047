// Stand-alone driver of fedm_amd/csrc/table_lookup.h for tests/test_table_lookup.py (host compiler, no HIP).
// stdin: n, then n knots, n values, m, then m arguments, all as C99 hex floats ("nan", "inf" included).
// stdout: per argument "segment value derivative", the numbers as hex floats.
#include <cstdio>
#include <vector>

#include "table_lookup.h"

int main() {
    int n = 0, m = 0;
    if (std::scanf("%d", &n) != 1 || n < 1) return 2;
    std::vector<double> x(n), y(n);
    for (int i = 0; i < n; ++i)
        if (std::scanf("%la", &x[i]) != 1) return 2;
    for (int i = 0; i < n; ++i)
        if (std::scanf("%la", &y[i]) != 1) return 2;
    if (std::scanf("%d", &m) != 1 || m < 0) return 2;
    for (int k = 0; k < m; ++k) {
        double E, val, der;
        if (std::scanf("%la", &E) != 1) return 2;
        // exact-size copies: an access outside [0, n) is an access outside the allocation (address sanitizer)
        std::vector<double> xs(x), ys(y);
        const int seg = fedm_table_segment(xs.data(), n, E);
        fedm_table_eval(xs.data(), ys.data(), n, E, &val, &der);
        std::printf("%d %a %a\n", seg, val, der);
    }
    return 0;
}
