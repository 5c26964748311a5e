// lsm2d_k_align_probe.h -- align_body's phase-probe macros (lsm2d_k_align.h; tools/phase_probe.py reads what they collect).  Empty statements unless the library is built with -DLSM2D_PHASE_PROBE.
// Part of lsm2d_kernels.h (included there, in front of lsm2d_k_align.h); not a translation unit of its own.  The macros expand inside align_body: `tid` and `s_ph` are its names.
// Diagnostics build: thread 0 sums the cycles it spends in the query / projection phase, at the barrier + reduction, and in the solve, into s_ph[0..2] (s_ph[3]: the last stamp).
// Every mode defines the same six macros.  LSM2D_PH(k): the three buckets' stamps; _LISTS / _STREAM: behind the unit lists, behind the stream; _SUMS / _TAIL: mode 4's;
// _CAND(k): the candidate lists' sections (modes 5 and 6; tools/phase_probe.py --lists): -1 a section begins, 0 / 1 / 2 a plain stream, a build iteration's stream, a gather ends, 3 / 4 a blockers pass, a collect pass ends
#define LSM2D_PH_NONE() do { } while (0)
#ifdef LSM2D_PHASE_PROBE
#define LSM2D_PH_STAMP(k) do { if (tid == 0) { const unsigned long long now__ = __builtin_amdgcn_s_memtime(); s_ph[k] += now__ - s_ph[3]; s_ph[3] = now__; } } while (0)
#define LSM2D_PH_SKIP() do { if (tid == 0) s_ph[3] = __builtin_amdgcn_s_memtime(); } while (0)      // what went before belongs to no bucket
// -DLSM2D_PHASE_PROBE=1 (or empty): the three buckets above.  =2: unit lists + stream | bin walk + reduction | solve + the rest.  =3: unit lists | stream | everything else.  =4: bin walk + wave sums | everything else | wave 0's stretch (a single slice).
#if LSM2D_PHASE_PROBE + 0 == 2
#define LSM2D_PH(k) LSM2D_PH_STAMP((k) == 0 ? 1 : (k))
#define LSM2D_PH_LISTS() LSM2D_PH_NONE()
#define LSM2D_PH_STREAM() LSM2D_PH_STAMP(0)
#define LSM2D_PH_SUMS() LSM2D_PH_NONE()
#define LSM2D_PH_TAIL() LSM2D_PH_NONE()
#define LSM2D_PH_CAND(k) LSM2D_PH_NONE()
#elif LSM2D_PHASE_PROBE + 0 == 3
#define LSM2D_PH(k) LSM2D_PH_STAMP(2)
#define LSM2D_PH_LISTS() LSM2D_PH_STAMP(0)
#define LSM2D_PH_STREAM() LSM2D_PH_STAMP(1)
#define LSM2D_PH_SUMS() LSM2D_PH_NONE()
#define LSM2D_PH_TAIL() LSM2D_PH_NONE()
#define LSM2D_PH_CAND(k) LSM2D_PH_NONE()
#elif LSM2D_PHASE_PROBE + 0 == 4      // bin walk + wave sums | everything else | wave 0's stretch behind the sums' barrier, up to the iteration's closing barrier
#define LSM2D_PH(k) LSM2D_PH_NONE()
#define LSM2D_PH_LISTS() LSM2D_PH_NONE()
#define LSM2D_PH_STREAM() LSM2D_PH_STAMP(1)
#define LSM2D_PH_SUMS() LSM2D_PH_STAMP(0)
#define LSM2D_PH_TAIL() LSM2D_PH_STAMP(2)
#define LSM2D_PH_CAND(k) LSM2D_PH_NONE()
#elif LSM2D_PHASE_PROBE + 0 == 5      // k_align_cand: the unit list's stream in an iteration that builds no list | the build iteration's stream (blockers included) | a list-served gather; the remainder of the lifetime is everything else
#define LSM2D_PH(k) LSM2D_PH_NONE()
#define LSM2D_PH_LISTS() LSM2D_PH_SKIP()
#define LSM2D_PH_STREAM() LSM2D_PH_NONE()
#define LSM2D_PH_SUMS() LSM2D_PH_NONE()
#define LSM2D_PH_TAIL() LSM2D_PH_NONE()
#define LSM2D_PH_CAND(k) do { if ((k) >= 0 && (k) <= 2) LSM2D_PH_STAMP((k) & 3); else LSM2D_PH_SKIP(); } while (0)
#elif LSM2D_PHASE_PROBE + 0 == 6      // k_align_cand: a blockers pass of its own (none since round 22) | the collect pass | unit-list rebuilds
#define LSM2D_PH(k) LSM2D_PH_NONE()
#define LSM2D_PH_LISTS() LSM2D_PH_STAMP(2)
#define LSM2D_PH_STREAM() LSM2D_PH_NONE()
#define LSM2D_PH_SUMS() LSM2D_PH_NONE()
#define LSM2D_PH_TAIL() LSM2D_PH_NONE()
#define LSM2D_PH_CAND(k) do { if ((k) == 3) LSM2D_PH_STAMP(0); else if ((k) == 4) LSM2D_PH_STAMP(1); else LSM2D_PH_SKIP(); } while (0)
#else
#define LSM2D_PH(k) LSM2D_PH_STAMP(k)
#define LSM2D_PH_LISTS() LSM2D_PH_NONE()
#define LSM2D_PH_STREAM() LSM2D_PH_NONE()
#define LSM2D_PH_SUMS() LSM2D_PH_NONE()
#define LSM2D_PH_TAIL() LSM2D_PH_NONE()
#define LSM2D_PH_CAND(k) LSM2D_PH_NONE()
#endif
#else
#define LSM2D_PH(k) LSM2D_PH_NONE()
#define LSM2D_PH_LISTS() LSM2D_PH_NONE()
#define LSM2D_PH_STREAM() LSM2D_PH_NONE()
#define LSM2D_PH_SUMS() LSM2D_PH_NONE()
#define LSM2D_PH_TAIL() LSM2D_PH_NONE()
#define LSM2D_PH_CAND(k) LSM2D_PH_NONE()
#endif
