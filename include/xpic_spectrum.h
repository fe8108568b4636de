/* xpic_spectrum.h -- field spectra on the device: the power |F^(k)|^2 of a scalar on the grid, its sums along the axes and
 * over shells of |k|, single modes, and a probe of modes that rides with xpic_step (an extension: the reference has no
 * spectral diagnostic).  Included by xpic_hip.h, which defines xpic_ctx; include that header.  (The entry
 * points stand here and in the package's SPECTRUM_PROTOTYPES; tests/test_abi_spectrum.py holds the two to each other.)
 *
 * The transform is xpic_poisson.h's: three dense float64 passes with the Hartley matrix H_n along x, y, z on the matrix
 * cores, the same kernel and the same tables.  They give the separable transform
 *     T(k) = sum_j x(j) cas(2 pi kx jx / nx) cas(2 pi ky jy / ny) cas(2 pi kz jz / nz) / sqrt(N),   cas = cos + sin,
 * which is not the 3-D Hartley transform.  With r_a the reflection k_a -> (n_a - k_a) mod n_a and r_xyz all three,
 *     H(k) = 1/2 [ T(r_x k) + T(r_y k) + T(r_z k) - T(r_xyz k) ],   H(-k) = H(r_xyz k),
 * and for the orthonormal DFT F^(k) = sum_j x(j) exp(-2 pi i k.j / n) / sqrt(N):
 *     Re F^ = (H(k) + H(-k)) / 2,   Im F^ = -(H(k) - H(-k)) / 2,   P(k) = |F^(k)|^2 = (H(k)^2 + H(-k)^2) / 2,
 * sum_k P(k) = sum_j x(j)^2 (Parseval).  The four terms are added in the written order for H(k) and for H(-k), without
 * contraction: P(k) and P(-k) are the same bits.  All float64, any extent, no complex arithmetic.
 *
 * Sources.  source >= 0: component comp (0, 1, 2) of the vector enum xpic_field `source`; the vectors are stored
 * component-planar, so the component is read in place.  XPIC_SPECTRUM_RHO: the charge density xpic_gauss_residual
 * deposits -- all sorts, second order, plus the background, the mean left in -- from the same deposit function (XPIC_W2 is
 * its scratch); comp is ignored.  XPIC_SPECTRUM_HOST: the scalar [nz][ny][nx] the caller hands in (scalar_zyx; ignored for
 * every other source); comp is ignored; the hook that pins the kernels, as xpic_poisson_apply pins the solve's.
 * Phases refer to the node index of the component's own array: the Yee stagger is not applied (a component that lives half
 * a cell along an axis carries the factor exp(-i k_a d_a / 2) there, which is left to the caller; |F^|^2 does not see it).
 *
 * xpic_spectrum_power: P [nz][ny][nx], index (kz, ky, kx), unfolded (index n_a - m is wavenumber -m).
 * xpic_spectrum: P is not stored; it is reduced to axis_a[k_a] = the sum of P over the other two indices (axis_x[nx],
 *   axis_y[ny], axis_z[nz]), to total = sum_k P, and to nshell shells of s = kx2[x] + ky2[y] + kz2[z] (two plain adds in
 *   that order), kx2[i] = k^2 of k = 2 pi m / (n_a d_a) with m = i folded to (-n_a/2, n_a/2], three tables built on the host.
 *   Shell j holds edges2[j] <= s < edges2[j+1]; edges2: nshell + 1 ascending SQUARED edges.  shell[nshell] the power,
 *   shell_count[nshell] the modes of each; a mode outside [edges2[0], edges2[nshell]) goes to no shell: outside2 = {its
 *   power, the count of such modes} (nshell = 0: every mode).  Any output pointer may be null, except that nshell > 0
 *   needs edges2 and shell.  The axis sums and the total are fixed-order reductions without floating-point atomics: the
 *   same bits twice.  The shells are summed with LDS atomics inside a workgroup and in a fixed order across workgroups:
 *   every term is >= 0, so any order is within terms * eps relative.
 * xpic_spectrum_modes: re_im[nmodes][2] = (Re, Im) F^ of the signed mode numbers modes_xyz[nmodes][3] (any integer; folded
 *   modulo the extent), from the same H(+-k) as the power.
 * The work planes are the Gauss vectors' (nothing carries state in them from one step to the next); the partial sums and the
 * probes' rows are the spectrum's own, made at first use and freed with the context.  A context that never asks for a
 * spectrum allocates and launches nothing for it.  xpic_set_poisson_solver's kind and xpic_gauss_info's counters are not
 * touched.
 *
 * Probes.  xpic_spectrum_probe_create: a passive probe of nmodes modes of (source, comp) -> id.  After every xpic_step whose
 * count (the steps this context has made) is a multiple of `every`, the probe runs on the fields the step leaves behind:
 * the order of the riders is the clean of xpic_set_gauss_clean, then the attached tracer sets, then the probes in creation
 * order.  It appends one row (step, Re and Im per mode) to a device buffer of `capacity` rows; a full buffer records nothing
 * more and counts `dropped`.  No host synchronisation of its own (XPIC_SPECTRUM_RHO has the deposit's).  A run with a
 * probe returns the same bits as one without -- fields, particles, iterations, xpic_gauss_info; the one exception is the
 * scratch vector XPIC_W2, which a probe of XPIC_SPECTRUM_RHO overwrites as every charge deposit does.  Ids are never given twice.  At most XPIC_SPECTRUM_MAX_PROBES live probes per context;
 * XPIC_SPECTRUM_HOST is not a probe source.
 * xpic_spectrum_probe_get: the first min(rows, recorded) rows -> step[rows], re_im[rows][nmodes][2] (either may be null);
 * *recorded, *dropped; reset != 0 empties the buffer and the counters afterwards.  xpic_spectrum_probe_destroy frees it.
 *
 * Refused, with a message and nothing changed: a null context; a context with ghost planes (z-slabs, self_ring included: a
 * transform along z needs every plane); an extent above XPIC_POISSON_MAX_EXTENT; an unknown source or an unallocated
 * field; XPIC_W2 as the source (the deposit's scratch); comp outside 0..2; a host scalar that is null or not finite; nshell < 0 or above XPIC_SPECTRUM_MAX_SHELLS;
 * edges2 not finite or not strictly ascending; nmodes < 1, every < 1, capacity < 1; an unknown or destroyed probe id. */
#ifndef XPIC_SPECTRUM_H
#define XPIC_SPECTRUM_H
#define XPIC_SPECTRUM_MAX_SHELLS 2048
#define XPIC_SPECTRUM_MAX_PROBES 16
enum xpic_spectrum_source { XPIC_SPECTRUM_HOST = 100, XPIC_SPECTRUM_RHO = 101 };
#ifdef __cplusplus
extern "C" {
#endif
int xpic_spectrum_power(xpic_ctx* ctx, int source, int comp, const double* scalar_zyx, double* power_zyx);
int xpic_spectrum(xpic_ctx* ctx, int source, int comp, const double* scalar_zyx, double* axis_x, double* axis_y,
                  double* axis_z, int nshell, const double* edges2, double* shell, int64_t* shell_count, double* outside2,
                  double* total);
int xpic_spectrum_modes(xpic_ctx* ctx, int source, int comp, const double* scalar_zyx, int nmodes, const int32_t* modes_xyz,
                        double* re_im);
int xpic_spectrum_probe_create(xpic_ctx* ctx, int source, int comp, int nmodes, const int32_t* modes_xyz, int every,
                               int64_t capacity, int* id);
int xpic_spectrum_probe_get(xpic_ctx* ctx, int id, int64_t rows, int64_t* step, double* re_im, int64_t* recorded,
                            int64_t* dropped, int reset);
int xpic_spectrum_probe_destroy(xpic_ctx* ctx, int id);
#ifdef __cplusplus
}
#endif
#endif
