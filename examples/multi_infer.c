/* Minimal C host for the multi-model API of libbitnetmcu_hip.so: two or more exporter-written headers,
 * one image file, every model's class ids from one call.
 *
 *   gcc -std=c99 -Iinclude examples/multi_infer.c -Lbitnetmcu_amd -lbitnetmcu_hip -Wl,-rpath,$PWD/bitnetmcu_amd -o multi_infer
 *   ./multi_infer images.i8 model_a.h model_b.h [...]        # images.i8: n x 256 int8 bytes (16x16 images, row-major)
 *
 * Prints one line per image: the class id of each model, in the order the headers were given, separated by blanks.  Needs an
 * MI355X; without a HIP device bnm_multi_create reports BNM_EHIP.
 */
#include <stdio.h>
#include <stdlib.h>
#include "bitnetmcu_hip.h"

static char *slurp(const char *path, size_t *len) {
    FILE *f = fopen(path, "rb");
    if (!f) return NULL;
    fseek(f, 0, SEEK_END);
    long n = ftell(f);
    fseek(f, 0, SEEK_SET);
    char *buf = (char *)malloc((size_t)n + 1);
    if (buf && fread(buf, 1, (size_t)n, f) != (size_t)n) { free(buf); buf = NULL; }
    fclose(f);
    if (buf) buf[n] = 0;
    *len = (size_t)n;
    return buf;
}

int main(int argc, char **argv) {
    if (argc < 4 || argc - 2 > 16) {
        fprintf(stderr, "usage: %s <images.i8> <BitNetMCU_model.h> <BitNetMCU_model.h> [... up to 16 headers]\n", argv[0]);
        return 2;
    }
    const uint32_t k = (uint32_t)(argc - 2);
    size_t ilen = 0;
    char *images = slurp(argv[1], &ilen);
    if (!images || ilen % 256 != 0) {
        fprintf(stderr, "cannot read %s (the image file must hold n x 256 bytes)\n", argv[1]);
        return 2;
    }
    bnm_model *models[16] = {NULL};
    for (uint32_t m = 0; m < k; m++) {
        size_t hlen = 0;
        char *header = slurp(argv[2 + m], &hlen);
        if (!header) {
            fprintf(stderr, "cannot read %s\n", argv[2 + m]);
            return 2;
        }
        int rc = bnm_model_from_header_text(header, hlen, &models[m]);
        free(header);
        if (rc != BNM_OK) {
            fprintf(stderr, "%s: %s\n", argv[2 + m], bnm_last_error());
            return 1;
        }
    }
    bnm_multi *mc = NULL;
    if (bnm_multi_create((const bnm_model *const *)models, k, -1, &mc) != BNM_OK) {
        fprintf(stderr, "%s\n", bnm_last_error());
        return 1;
    }
    const uint64_t n = ilen / 256;
    uint32_t *cls = (uint32_t *)malloc((size_t)(n * k + 1) * sizeof(uint32_t));      /* [k][n] */
    if (!cls || bnm_multi_infer_host(mc, (const int8_t *)images, n, cls, NULL) != BNM_OK) {
        fprintf(stderr, "%s\n", bnm_last_error());
        return 1;
    }
    for (uint64_t i = 0; i < n; i++)
        for (uint32_t m = 0; m < k; m++) printf(m + 1 < k ? "%u " : "%u\n", cls[(uint64_t)m * n + i]);
    bnm_multi_destroy(mc);
    for (uint32_t m = 0; m < k; m++) bnm_model_free(models[m]);
    free(cls);
    free(images);
    return 0;
}
