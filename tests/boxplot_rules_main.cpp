// Host program of tests/test_boxplot_rules_host.py: the scalar rules of csrc/boxplot.h applied to the inputs of a file,
// one request per line, every double and float as the hexadecimal of its bits.
//
//   K <double>            -> key, value of the key
//   F <float>             -> key, value of the key (a double)
//   L <q1> <q3>           -> lower limit, upper limit
//   Z <rank> <nneg> <nzero>  (decimal) -> settled, key, rank left, equal
//   S <n> <double> x n    -> q1, median, q3, lower limit, upper limit, whisker_lo, whisker_hi, fliers (decimal)
//
// The sample's order statistics come from a sort by the ordered keys: the rules do the rest as a kernel does.
#include "boxplot.h"

#include <algorithm>
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

using namespace revs;

static uint64_t bits(double v) { uint64_t u; memcpy(&u, &v, 8); return u; }
static double dbl(uint64_t u) { double v; memcpy(&v, &u, 8); return v; }

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    FILE *f = fopen(argv[1], "r");
    if (!f) return 2;
    char op;
    while (fscanf(f, " %c", &op) == 1) {
        if (op == 'K') {
            uint64_t u;
            if (fscanf(f, "%" SCNx64, &u) != 1) return 3;
            const unsigned long long k = box_key(dbl(u));
            printf("%016llx %016" PRIx64 "\n", k, bits(box_val(k)));
        } else if (op == 'F') {
            unsigned u;
            if (fscanf(f, "%x", &u) != 1) return 3;
            const unsigned k = box_key_f(u);
            printf("%08x %016" PRIx64 "\n", k, bits(box_val_f(k)));
        } else if (op == 'L') {
            uint64_t a, b;
            if (fscanf(f, "%" SCNx64 " %" SCNx64, &a, &b) != 2) return 3;
            double lo, hi;
            box_limits(dbl(a), dbl(b), lo, hi);
            printf("%016" PRIx64 " %016" PRIx64 "\n", bits(lo), bits(hi));
        } else if (op == 'Z') {
            unsigned rank, nneg, nzero, ans = 0u, left = 0u, eq = 0u;
            if (fscanf(f, "%u %u %u", &rank, &nneg, &nzero) != 3) return 3;
            const bool settled = box_settled_at_zero(rank, nneg, nzero, ans, left, eq);
            printf("%d %08x %u %u\n", settled ? 1 : 0, ans, left, eq);
        } else if (op == 'S') {
            unsigned n;
            if (fscanf(f, "%u", &n) != 1 || n == 0) return 3;
            std::vector<unsigned long long> key(n);
            for (unsigned i = 0; i < n; ++i) {
                uint64_t u;
                if (fscanf(f, "%" SCNx64, &u) != 1) return 3;
                key[i] = box_key(dbl(u));
            }
            std::sort(key.begin(), key.end());
            double q[3];
            for (int e = 0; e < 3; ++e) {
                unsigned rank, rem4;
                box_rank(n, e + 1, rank, rem4);
                const unsigned cle = (unsigned)(std::upper_bound(key.begin(), key.end(), key[rank]) - key.begin());
                const double lo = box_val(key[rank]);
                // (the smallest key above: what the neighbour walks find)
                const double hi = box_next_differs(rank, n, cle) ? box_val(key[cle]) : lo;
                q[e] = box_quartile(lo, hi, rem4);
            }
            double lim_lo, lim_hi, cand_lo = 0.0, cand_hi = 0.0;
            box_limits(q[0], q[2], lim_lo, lim_hi);
            bool any_lo = false, any_hi = false;
            for (unsigned i = 0; i < n; ++i) {
                const double v = box_val(key[i]);
                if (v >= lim_lo && !any_lo) { any_lo = true; cand_lo = v; }
                if (v <= lim_hi) { any_hi = true; cand_hi = v; }
            }
            const double wlo = box_whisker_lo(q[0], any_lo, cand_lo), whi = box_whisker_hi(q[2], any_hi, cand_hi);
            unsigned fl = 0;
            for (unsigned i = 0; i < n; ++i) fl += box_is_flier(box_val(key[i]), wlo, whi) ? 1u : 0u;
            printf("%016" PRIx64 " %016" PRIx64 " %016" PRIx64 " %016" PRIx64 " %016" PRIx64 " %016" PRIx64 " %016" PRIx64 " %u\n",
                   bits(q[0]), bits(q[1]), bits(q[2]), bits(lim_lo), bits(lim_hi), bits(wlo), bits(whi), fl);
        } else {
            return 3;
        }
    }
    fclose(f);
    return 0;
}
