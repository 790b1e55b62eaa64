// Host check of tbx_isqrt (toybox_amd/csrc/tbx_common.hpp), built and run by tests/test_tree_act.py: the function is __host__
// __device__, so the host compiler's copy is the text the kernels run.  Prints one line per mismatch against an integer root found
// by bisection, for every argument the tree can ask for -- n << 16 with n in 0 .. 5120 -- and for the squares around them.
#include "../toybox_amd/csrc/tbx_common.hpp"
#include <cstdio>

static long long root_by_bisection(long long x)
{
    long long lo = 0, hi = 3037000499ll;      // floor(sqrt(2^63 - 1))
    while (lo < hi) {
        const long long mid = lo + (hi - lo + 1) / 2;
        if (mid * mid <= x) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

int main()
{
    int bad = 0;
    long long checked = 0;
    auto check = [&](long long x) {
        if (x < 0) return;
        const long long got = tbx_isqrt(x), want = root_by_bisection(x);
        checked++;
        if (got != want) {
            bad++;
            printf("isqrt(%lld) = %lld, want %lld\n", x, got, want);
        }
    };
    for (long long n = 0; n <= 5120; n++) check(n << 16);
    for (long long r = 0; r <= 18400; r++)      // 18400^2 > 5120 << 16: every square in range, and its neighbours
        for (long long d = -1; d <= 1; d++) check(r * r + d);
    for (long long r = 94906265ll - 2000; r <= 94906265ll; r++)      // up to 2^53, far beyond the tree's arguments
        for (long long d = -1; d <= 1; d++) check(r * r + d);
    printf("checked %lld bad %d\n", checked, bad);
    return bad ? 1 : 0;
}
