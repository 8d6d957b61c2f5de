/*
 * shim_rng.c -- the five GSL generator calls of sampletau/c_sample_tau.c, forwarded to the oracle's MT19937.
 * TEST INFRASTRUCTURE ONLY (oracle/Makefile: ref -> oracle/_ref/libref_sampletau.so).
 *
 * The reference's sweep uses GSL for its generator and for nothing else (c_sample_tau.c:26-45, :174); all of
 * its arithmetic is its own plain C.  This file lets that C file compile, unmodified, without GSL: what is
 * compared against the oracle and the device is then the reference's own code, and the only stand-in is the
 * uniform stream -- which is orc_mt (desman_oracle.c), pinned bit for bit against numpy's legacy MT19937 raw
 * stream (tests/test_oracle_golden.py) and against the device generator.  No second MT19937 is written here.
 *
 * Behaviour, from the GSL manual:
 *   gsl_rng_env_setup   reads GSL_RNG_TYPE / GSL_RNG_SEED into the library defaults and returns the default
 *                       type.  The reference ignores the result and names its type explicitly, so the type
 *                       variable has no effect on it.  GSL_RNG_SEED would move the default seed below; this
 *                       stand-in does not read it (neither do the oracle's orc_initRNG and the product's
 *                       dsm_initRNG): the default seed is always 0.
 *   gsl_rng_alloc       a new generator of the given type, seeded with the default seed (0).
 *   gsl_rng_set         seeds it; for mt19937 seed 0 stands for 4357 (orc_mt_seed).
 *   gsl_rng_uniform     a double in [0, 1): for mt19937 the 32-bit word divided by 2^32.
 *   gsl_rng_free        releases it.
 */
#include <stdlib.h>

#include <gsl/gsl_rng.h>

#include "../orc_mt.h"

struct gsl_rng_type { const char *name; };
struct gsl_rng { orc_mt mt; };

static const gsl_rng_type mt19937_type = { "mt19937" };
const gsl_rng_type *gsl_rng_mt19937 = &mt19937_type;

const gsl_rng_type *gsl_rng_env_setup(void) { return gsl_rng_mt19937; }

gsl_rng *gsl_rng_alloc(const gsl_rng_type *T)
{
    if (T != gsl_rng_mt19937) return NULL;          /* the only type this stand-in knows */
    gsl_rng *r = (gsl_rng *)malloc(sizeof(gsl_rng));
    if (r) orc_mt_seed(&r->mt, 0);
    return r;
}

void gsl_rng_set(const gsl_rng *r, unsigned long int seed) { orc_mt_seed((orc_mt *)&r->mt, seed); }

double gsl_rng_uniform(const gsl_rng *r) { return orc_mt_uniform((orc_mt *)&r->mt); }

void gsl_rng_free(gsl_rng *r) { free(r); }
