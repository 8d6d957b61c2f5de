/* gsl/gsl_randist.h -- empty on purpose: sampletau/c_sample_tau.c includes this header and uses nothing from it
 * (oracle/gsl_shim/shim_rng.c says what the stand-in is for). */
