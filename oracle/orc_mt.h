/* orc_mt.h -- the oracle's MT19937 (GSL flavour), defined in desman_oracle.c.  TEST INFRASTRUCTURE ONLY.
 * Shared with oracle/gsl_shim/shim_rng.c so that the build of the reference's own sweep (oracle/_ref) draws
 * from this generator and no second one exists. */
#ifndef ORC_MT_H
#define ORC_MT_H
#include <stdint.h>

typedef struct {
    uint32_t mt[624];
    int pos;
} orc_mt;

void orc_mt_seed(orc_mt *r, unsigned long seed);       /* seed 0 -> 4357, as gsl_rng_set(mt19937, 0) */
uint32_t orc_mt_u32(orc_mt *r);
double orc_mt_uniform(orc_mt *r);                      /* word / 2^32, in [0, 1) */
void orc_mt_fill_u32(orc_mt *r, uint32_t *out, long n);

#endif
