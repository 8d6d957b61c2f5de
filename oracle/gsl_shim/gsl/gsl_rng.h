/* gsl/gsl_rng.h -- stand-in for the one GSL header sampletau/c_sample_tau.c uses something from.
 *
 * Written from the GSL manual's description of the random number generator interface ("Random number
 * generator initialization", "Sampling from a random number generator", "Random number environment
 * variables"); nothing here is copied from GSL.  Only what that file calls is declared: five functions
 * and the generator type gsl_rng_mt19937.  Both types stay opaque -- the caller holds pointers only.
 * Implemented in oracle/gsl_shim/shim_rng.c on top of the oracle's MT19937 (oracle/orc_mt.h).
 *
 * TEST INFRASTRUCTURE ONLY: used to compile oracle/_ref/libref_sampletau.so (oracle/Makefile: ref).
 */
#ifndef ORC_GSL_SHIM_RNG_H
#define ORC_GSL_SHIM_RNG_H

typedef struct gsl_rng_type gsl_rng_type;
typedef struct gsl_rng gsl_rng;

extern const gsl_rng_type *gsl_rng_mt19937;

const gsl_rng_type *gsl_rng_env_setup(void);
gsl_rng *gsl_rng_alloc(const gsl_rng_type *T);
void gsl_rng_set(const gsl_rng *r, unsigned long int seed);
double gsl_rng_uniform(const gsl_rng *r);
void gsl_rng_free(gsl_rng *r);

#endif
