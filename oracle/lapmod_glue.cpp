// C entry points of oracle/_ref/liblapmod_ref.so (test infrastructure; oracle/Makefile compiles this file together
// with the reference's LAP/_lapjv_cpp/lapmod.cpp where the reference exists).
//   lapmod_c: the reference's lapmod_internal behind an unmangled name.
//   lapmod_v: the same three phases, called as lapmod_internal calls them, with v owned by the caller so that the
//             final column duals can be stored (tests/golden/make_lapmod.py).
#include <vector>
#include "lapjv.h"
int_t _ccrrt_sparse(const uint_t, cost_t *, uint_t *, uint_t *, int_t *, int_t *, int_t *, cost_t *);
int_t _carr_sparse(const uint_t, cost_t *, uint_t *, uint_t *, const uint_t, int_t *, int_t *, int_t *, cost_t *);
int_t _ca_sparse(const uint_t, cost_t *, uint_t *, uint_t *, const uint_t, int_t *, int_t *, int_t *, cost_t *, int);
extern "C" int lapmod_c(unsigned n, double *cc, unsigned *ii, unsigned *kk, int *x, int *y, int fp)
{ return lapmod_internal(n, cc, ii, kk, x, y, (fp_t)fp); }
extern "C" int lapmod_v(unsigned n, double *cc, unsigned *ii, unsigned *kk, int *x, int *y, double *v, int fp)
{ std::vector<int_t> fr(n); int ret = _ccrrt_sparse(n, cc, ii, kk, fr.data(), x, y, v);
  for (int i = 0; ret > 0 && i < 2; ++i) ret = _carr_sparse(n, cc, ii, kk, ret, fr.data(), x, y, v);
  if (ret > 0) ret = _ca_sparse(n, cc, ii, kk, ret, fr.data(), x, y, v, fp);
  return ret; }
