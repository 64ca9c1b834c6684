/* ictr_c2f_set.h -- a lockstep set of coarse-to-fine dense flows (ictr_c2fflow.hip; DESIGN.md §4 "Lockstep sets"). Part
 * of ictr.h, which includes it inside its extern "C" block; not
 * to be included alone. It is a file of its own because tests/test_c2fflow_cpu.py pins the list of ictr_c2fflow_*
 * declarations in ictr.h's own text; the ctypes table of these is _lib.SIGNATURES_SET. */
#ifndef ICTR_C2F_SET_H
#define ICTR_C2F_SET_H
/* A set runs n (1 .. ICTR_C2FSET_MAX) ictr_c2fflow objects of equal shape and parameters in lockstep: per level and stage
 * ONE launch covers all members, the member index a grid dimension. There is no new arithmetic: a lockstep run on the
 * pairs (pyr_a[m], pyr_b[m]) leaves member m in exactly the state its own ictr_c2fflow_run(pyr_a[m], pyr_b[m]) would have
 * left it in -- every level's node displacements, status, node bias and field, the result plane, what ictr_c2fflow_result,
 * _device_ptr, _read_level and _read_level_bias(_rgb) return -- except that the member's ictr_c2fflow_get_kernel_ms and
 * _get_upsample_ms return zeros (the stage times are the set's). The set holds its members' addresses and owns none of
 * them: they outlive it, or at least its last run.
 * Refused with a message that names the member and the field, the set and every member unchanged: n outside
 * 1 .. ICTR_C2FSET_MAX, a NULL member or set, the same object twice, members that differ from member 0 in w, h, lv_f, lv_l,
 * step, psz, maxiter, eps, the densifier's minerr or power, refinement on or off or its alpha, gamma, delta, n_outer, n_sor,
 * omega, patnorm, x_only, channels, cost or huber_k; ictr_c2fset_run on a 3-channel set and ictr_c2fset_run_rgb on a grey
 * one; pyramids whose levels are not the members' size (every check of ictr_c2fflow_run, per member). The members are
 * compared at every run: their setters may be called between runs. Two members may read the same pyramid. */
enum { ICTR_C2FSET_MAX = 8 };
typedef struct ictr_c2fset ictr_c2fset;
int ictr_c2fset_create(ictr_c2fset **out, ictr_c2fflow *const *members, int n);
void ictr_c2fset_destroy(ictr_c2fset *s);
/* grey members: pyr_a[m], pyr_b[m] are member m's frames. Everything is enqueued on hip_stream; nothing is waited for. */
int ictr_c2fset_run(ictr_c2fset *s, const ictr_pyramid *const *pyr_a, const ictr_pyramid *const *pyr_b, void *hip_stream);
/* 3-channel members: pyr_a[3 * m + ch], pyr_b[3 * m + ch] are channel ch of member m's frames */
int ictr_c2fset_run_rgb(ictr_c2fset *s, const ictr_pyramid *const *pyr_a, const ictr_pyramid *const *pyr_b,
                        void *hip_stream);
int ictr_c2fset_size(const ictr_c2fset *s, int *n);
/* kernel launches plus memsets the last run enqueued (0 before the first). It does not depend on n. (With the refinement
 * at n_outer = 0, which copies each member's field, the n copies are counted.) */
int ictr_c2fset_last_operations(const ictr_c2fset *s, int *ops);
/* timing on: the next runs record events around the stages. ms [lv_f + 1][3] of the last run (waits for it), per level
 * the search with its fill, the densification and the refinement, each for the whole set; zeros without timing and for
 * the levels below lv_l. upsample_ms (may be NULL): the up-sampling of a set with lv_l > 0. */
int ictr_c2fset_set_timing(ictr_c2fset *s, int on);
int ictr_c2fset_get_kernel_ms(ictr_c2fset *s, float *ms, float *upsample_ms);
#endif /* ICTR_C2F_SET_H */
