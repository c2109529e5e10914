/* mxs_operands_san.c -- TEST INFRASTRUCTURE (tests/test_mxs_operand_tiles.py): k_mxs's device
 * operand tiles (jx_mxs_device_operands, csrc/jpgx_plan.cpp) under -fsanitize=address,undefined, as
 * a program of its own: the hook writes into an exact-size heap buffer (a byte past either end is
 * an AddressSanitizer report) and the three tiles are held against the plan's six.
 * Exit status 0 and "mxs_operands_san: clean" when everything holds. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "jpgx_compat.h"
#include "../../jpeg-encoder-and-decoder_amd/csrc/jpgx_internal.h"

#define CHECK(c)                                                              \
    do {                                                                      \
        if (!(c)) {                                                           \
            fprintf(stderr, "mxs_operands_san: line %d: %s\n", __LINE__, #c); \
            return 1;                                                         \
        }                                                                     \
    } while (0)

typedef uint16_t tile[64][8];

int main(void)
{
    CHECK(jx_mx_parts() == 2);
    tile *ops = (tile *)malloc(3 * JX_MX_PARTS * sizeof(tile));        /* exact sizes */
    tile *dev = (tile *)malloc(3 * sizeof(tile));
    CHECK(ops && dev);
    memset(dev, 0xA5, 3 * sizeof(tile));
    CHECK(jx_mx_operands(ops) == 0);
    CHECK(jx_mxs_device_operands(dev) == 0);
    CHECK(memcmp(dev[0], ops[0], sizeof(tile)) == 0);
    CHECK(memcmp(dev[1], ops[3], sizeof(tile)) == 0);
    int nonzero[2] = {0, 0};
    for (int l = 0; l < 64; l++)
        for (int e = 0; e < 8; e++) {
            const int lo = (l & 15) >= 8;
            CHECK(dev[2][l][e] == (lo ? ops[5][l][e] : ops[1][l][e]));
            /* the halves the tile drops are the plan's stored zeros */
            CHECK((lo ? ops[1][l][e] : ops[2][l][e]) == 0 && (lo ? ops[4][l][e] : ops[5][l][e]) == 0);
            nonzero[lo] += dev[2][l][e] != 0;
        }
    CHECK(nonzero[0] > 8 * 24 / 2 && nonzero[1] > 8 * 24 / 2);          /* both halves carry a matrix */
    /* a second call gives the same bytes (no state) */
    tile *again = (tile *)malloc(3 * sizeof(tile));
    CHECK(again);
    CHECK(jx_mxs_device_operands(again) == 0);
    CHECK(memcmp(again, dev, 3 * sizeof(tile)) == 0);
    free(again);
    free(dev);
    free(ops);
    printf("mxs_operands_san: clean\n");
    return 0;
}
