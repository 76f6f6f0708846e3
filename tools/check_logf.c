/* Exhaustive check of the logf restatement (xrt_logf in
 * simpleraytracing_amd/csrc/kernels/xrt_device.h): its
 * algorithm and constants -- this file's own copy -- with every f64 operation
 * rounded on its own, against the system libm's logf on all 2^32 inputs; NaNs
 * are compared by class.  Build without contraction, so that no step is fused:
 *
 *   gcc -O2 -ffp-contract=off -o check_logf tools/check_logf.c -lm -lpthread
 *
 * Prints the mismatch count; exit status 0 iff it is zero. */
#include <math.h>
#include <pthread.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

static float f32(uint32_t b) { float x; memcpy(&x, &b, 4); return x; }
static uint32_t bits(float x) { uint32_t b; memcpy(&b, &x, 4); return b; }

static const double Ln2 = 0x1.62e42fefa39efp-1;
static const double A0 = -0x1.00ea348b88334p-2, A1 = 0x1.5575b0be00b6ap-2, A2 = -0x1.ffffef20a4123p-2;
static const struct { double invc, logc; } T[16] = {
    {0x1.661ec79f8f3bep+0, -0x1.57bf7808caadep-2}, {0x1.571ed4aaf883dp+0, -0x1.2bef0a7c06ddbp-2},
    {0x1.49539f0f010b0p+0, -0x1.01eae7f513a67p-2}, {0x1.3c995b0b80385p+0, -0x1.b31d8a68224e9p-3},
    {0x1.30d190c8864a5p+0, -0x1.6574f0ac07758p-3}, {0x1.25e227b0b8ea0p+0, -0x1.1aa2bc79c8100p-3},
    {0x1.1bb4a4a1a343fp+0, -0x1.a4e76ce8c0e5ep-4}, {0x1.12358f08ae5bap+0, -0x1.1973c5a611cccp-4},
    {0x1.0953f419900a7p+0, -0x1.252f438e10c1ep-5}, {0x1p+0, 0x0p+0},
    {0x1.e608cfd9a47acp-1, 0x1.aa5aa5df25984p-5},  {0x1.ca4b31f026aa0p-1, 0x1.c5e53aa362eb4p-4},
    {0x1.b2036576afce6p-1, 0x1.526e57720db08p-3},  {0x1.9c2d163a1aa2dp-1, 0x1.bc2860d224770p-3},
    {0x1.886e6037841edp-1, 0x1.1058bc8a07ee1p-2},  {0x1.767dcf5534862p-1, 0x1.4043057b6ee09p-2},
};

static float restated_logf(float x)
{
    uint32_t ix = bits(x);
    if (ix == 0x3f800000u) return 0.0f;
    if (ix - 0x00800000u >= 0x7f800000u - 0x00800000u) {
        if (ix * 2u == 0u) return -INFINITY;
        if (ix == 0x7f800000u) return x;
        if ((ix & 0x80000000u) || ix * 2u >= 0xff000000u) return NAN;
        ix = bits(x * 0x1p23f);                          /* subnormal: normalise */
        ix -= 23u << 23;
    }
    const uint32_t tmp = ix - 0x3f330000u;
    const uint32_t i = (tmp >> 19) % 16u;
    const int32_t k = (int32_t)tmp >> 23;                /* arithmetic */
    const uint32_t iz = ix - (tmp & 0xff800000u);
    const double z = (double)f32(iz);
    const double r = z * T[i].invc - 1.0;
    const double y0 = T[i].logc + (double)k * Ln2;
    const double r2 = r * r;
    double y = A1 * r + A2;
    y = A0 * r2 + y;
    y = y * r2 + (y0 + r);
    return (float)y;
}

#define THREADS 8
static uint64_t bad[THREADS];

static void* sweep(void* arg)
{
    const uint64_t t = (uint64_t)(uintptr_t)arg, span = (1ull << 32) / THREADS;
    uint64_t n = 0;
    for (uint64_t u = t * span; u < (t + 1) * span; ++u) {
        const float x = f32((uint32_t)u);
        volatile float xv = x;                           /* the libm call itself, not a folded constant */
        const float a = restated_logf(x), c = logf(xv);
        if (bits(a) != bits(c) && !(isnan(a) && isnan(c))) n++;
    }
    bad[t] = n;
    return NULL;
}

int main(void)
{
    pthread_t th[THREADS];
    uint64_t total = 0;
    for (uintptr_t t = 0; t < THREADS; ++t)
        if (pthread_create(&th[t], NULL, sweep, (void*)t)) return 2;
    for (int t = 0; t < THREADS; ++t) {
        pthread_join(th[t], NULL);
        total += bad[t];
    }
    printf("logf mismatches %llu of 4294967296\n", (unsigned long long)total);
    return total ? 1 : 0;
}
