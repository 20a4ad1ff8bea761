/* vdjx_env.h -- the one place that reads the VDJX_* / VDJH_* environment variables (README.md lists them), for the HIP library and
 * the plain-C host sources alike.  No state: a caller that wants a variable read once keeps the answer in a function-local static. */
#ifndef VDJX_ENV_H
#define VDJX_ENV_H

#include <errno.h>
#include <stdio.h>
#include <stdlib.h>

/* the variable's text, NULL when it is not set (file names, "rank,nranks", a transport's name) */
static inline const char* vdjx_env_str(const char* name) { return getenv(name); }

/* the variable is present, whatever it holds */
static inline int vdjx_env_set(const char* name) { return getenv(name) != NULL; }

/* unset: dflt.  Set: the whole text as a decimal integer in [lo, hi] (0 is a value like any other); anything else -- empty, trailing
 * junk, out of range -- is named on stderr and dflt is used. */
static inline long long vdjx_env_num(const char* name, long long dflt, long long lo, long long hi) {
	const char* v = getenv(name);
	if (!v) return dflt;
	char* end = NULL;
	errno = 0;
	const long long x = strtoll(v, &end, 10);
	const int digits = (v[0] >= '0' && v[0] <= '9') || (v[0] == '-' && v[1] >= '0' && v[1] <= '9');      /* (strtoll would skip blanks and take a '+') */
	if (digits && *end == 0 && errno == 0 && x >= lo && x <= hi) return x;
	fprintf(stderr, "[vdjx] %s=\"%s\" ignored: not an integer in [%lld, %lld]; using %lld\n", name, v, lo, hi, dflt);
	return dflt;
}

#endif
