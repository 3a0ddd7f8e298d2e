/* nonfinite_oracle_cpu.c -- the CPU oracle on flow fields with NaN, Inf and out-of-int32 vectors, as a stand-alone
 * program for AddressSanitizer and UBSan (with float-cast-overflow): tests/test_nonfinite_cases_host.py writes the cases of
 * tests/nonfinite_cases.py into a file, this program runs every oracle entry the GPU tests compare against over them.
 *
 * File: records of  int32 H, W;  float fa[H*W*2];  float fb[H*W*2];  uint8 ma[H*W];  uint8 mb[H*W]  until the end.
 * Prints "<n> records ok" and a checksum of the validity masks.
 */
#include "../../oracle/ofl_oracle.c"
#include <stdio.h>

static void *need(size_t n)
{
    void *p = malloc(n ? n : 1);
    if (!p) { fprintf(stderr, "out of memory\n"); exit(2); }
    return p;
}

static int read_all(FILE *f, void *dst, size_t n) { return fread(dst, 1, n, f) == n; }

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: %s cases.bin\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    int records = 0;
    unsigned long sum = 0;
    int32_t hw[2];
    while (fread(hw, sizeof hw, 1, f) == 1) {
        const int H = hw[0], W = hw[1];
        if (H <= 0 || W <= 0 || H > 32766 || W > 32766) { fprintf(stderr, "bad record %d: %d x %d\n", records, H, W); return 2; }
        const size_t n = (size_t)H * W;
        float *fa = need(n * 8), *fb = need(n * 8), *out = need(n * 8), *g32 = need(n * 8);
        uint8_t *ma = need(n), *mb = need(n), *mout = need(n), *g8 = need(n);
        if (!read_all(f, fa, n * 8) || !read_all(f, fb, n * 8) || !read_all(f, ma, n) || !read_all(f, mb, n)) {
            fprintf(stderr, "short record %d\n", records);
            return 2;
        }
        for (int quant = 0; quant < 2; ++quant)
            for (int sign = -1; sign <= 1; sign += 2) {
                if (orc_compose3(fa, ma, fb, mb, sign, H, W, out, mout, quant)) return 1;
                for (size_t i = 0; i < n; ++i) sum += mout[i];
                /* K1 / K12 / K13: the vectors of fa as a two-channel float image, the mask bytes as a uint8 image */
                if (orc_gather_bilinear(fa, ORC_F32, 2, H, W, fb, H, W, 0, 0, sign, ma, g32, mout, quant, ORC_ARITH_NATIVE, ORC_RULE_EQ1)) return 1;
                for (size_t i = 0; i < n; ++i) sum += mout[i];
                for (int arith = 0; arith < 2; ++arith)
                    for (int rule = 0; rule < 3; ++rule) {
                        if (orc_gather_bilinear(ma, ORC_U8, 1, H, W, fb, H, W, 0, 0, sign, NULL, g8, mout, quant, arith, rule)) return 1;
                        for (size_t i = 0; i < n; ++i) sum += mout[i] + g8[i];
                    }
            }
        /* a flow smaller than the image: the field's first rows and columns at (1, 1) of the frame */
        if (H > 2 && W > 2) {
            if (orc_gather_bilinear(fa, ORC_F32, 2, H, W, fb, H - 2, W - 2, 1, 1, -1, ma, g32, mout, 0, ORC_ARITH_NATIVE, ORC_RULE_EQ1)) return 1;
            for (size_t i = 0; i < n; ++i) sum += mout[i];
        }
        sum += (unsigned long)orc_is_zero(fb, mb, n, 1, 1e-3) + (unsigned long)orc_is_zero(fb, NULL, n, 0, 1e-3);
        {   /* K6: the values travel, the addresses do not depend on them */
            const int Ho = (H * 3 + 1) / 2, Wo = (W * 3 + 1) / 2;
            float *r = need((size_t)Ho * Wo * 8);
            uint8_t *rm = need((size_t)Ho * Wo);
            if (orc_resize_flow(fb, mb, H, W, Ho, Wo, (double)H / Ho, (double)W / Wo, 1.5f, 1.5f, r, rm)) return 1;
            for (size_t i = 0; i < (size_t)Ho * Wo; ++i) sum += rm[i];
            free(r); free(rm);
        }
        free(fa); free(fb); free(out); free(g32); free(ma); free(mb); free(mout); free(g8);
        ++records;
    }
    fclose(f);
    printf("checksum %lu\n%d records ok\n", sum, records);
    return 0;
}
