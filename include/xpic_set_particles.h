/* xpic_set_particles.h -- SetParticles on the device.  Included by xpic_hip.h, which defines xpic_set_particles_params and
 * the enums; include that header.  (The two entry points stand here and in the package's LOAD_PROTOTYPES, not in
 * xpic_hip.h and PROTOTYPES: tests/test_abi.py holds those two to a fixed list of calls on a null context, and
 * tests/test_abi_set_particles.py holds these two to the same rules.)
 *
 * xpic_set_particles is SetParticles::execute (src/commands/set_particles.cpp:19-43) for the particles
 * particle0 .. particle0 + n - 1 of one command: each draws its coordinate, then its momentum, and is added iff its
 * coordinate lies in the local box (Particles::add_particle, src/interfaces/particles.cpp:47-67).  *added = particles
 * added, *energy = sum of 0.5 m |p|^2 n/Np over them (Energy::get_kinetic), both summed over the z-slabs (the call is
 * collective).
 * Coordinate generators (src/utils/particles_load.cpp:6-44, draws in the reference's order): PreciseCoordinate,
 * CoordinateInBox, CoordinateInCylinder as xpic_inject_particles has them, and CoordinateOnAnnulus:
 * r = sqrt(inner^2 + (outer^2 - inner^2) u), phi = 2 pi u, z = center z + height (u - 0.5).
 * Momentum generators (:47-125): PreciseMomentum and MaxwellianMomentum as xpic_inject_particles has them (per axis the
 * phase draw, then the amplitude draw), and
 *  - MaxwellCosinePerturbation: the thermal part sin(2 pi u) sqrt(-2 (T m / mec2) ln u) per axis, WITHOUT px, py, pz, is
 *    always divided by sqrt(m^2 + p^2); then v0[a] cos(2 pi wave_number[a] r[a] / L[a]) is added, v0[a] = amplitude[a]
 *    sqrt(T[a] / (m mec2)), r the particle's coordinate.  L is the extent of THIS call's box6.  (The reference keeps L in
 *    `static const` locals, :80-82: the first generator that runs freezes its box for the whole process.  A call here takes
 *    its own box.)
 *  - AngularMomentum as written: the three draws sqrt(-2 (T m / mec2) ln u) carry NO phase factor, so the thermal part is
 *    non-negative; with (x, y) = r - center and rr = hypot(x, y) the momentum is (-px y / rr, +py x / rr, pz) plus the
 *    thermal part, and where 1 / rr is infinite (a particle on the axis) it is (0, 0, pz) plus the thermal part.
 * The reference's JSON builder offers neither CoordinateOnAnnulus nor AngularMomentum (particles_builder.cpp:19-37,
 * 46-68); the host executable takes them only on a "device": true entry.
 * Stream: particle p draws from the counter-based stream of xpic_inject_particles' pair p under the same (seed, step):
 * this build's own RNG, not the reference's mt19937.  The draws depend on neither the slab decomposition, particle0 nor
 * chunk; every z-slab draws all n particles and keeps those in its planes.
 * Guarantees: (a) new records follow their cell's old records, which keep their bits and their order; the order among a
 * cell's new records is unspecified, their multiset is deterministic.  (b) Calls compose: (n, particle0 = 0) gives the same
 * per-cell multisets, *added and (to the rounding of the sum) *energy as (n1, 0) followed by (n - n1, n1).  (c) chunk
 * changes the launches and nothing else (the energy to the rounding of its sum).  (d) With a precise, box or cylinder
 * coordinate and a precise or Maxwellian momentum the new records are those of the ionized sort of xpic_inject_particles
 * with the same (seed, step, n), bit for bit, as sorted multisets per cell.  (e) Refused on every slab, before any sort
 * changes, with "xpic_set_particles" in the message: a bad sort, a null pointer, an unknown kind, negative n, particle0 or
 * chunk, outer_r < inner_r, a negative radius, non-finite geometry, a sort without mass or Np, and more records than the
 * sort's capacity or than 2^31 - 648 (the cells' counts and offsets are int).  (f) n == 0 launches nothing and returns
 * zeros.
 * Scratch: two passes over the particles, each in chunks of `chunk` (0: XPIC_SET_PARTICLES_CHUNK) particles, one launch per
 * chunk.  The first counts the new records of every cell (all chunks, before the first write: the capacity is known
 * before anything changes); the second draws the particles again and writes each behind its cell's old records, in a slot
 * taken from a per-cell cursor.  There is no per-particle scratch: the call holds two ints per cell. */
#ifndef XPIC_SET_PARTICLES_H
#define XPIC_SET_PARTICLES_H
#ifdef __cplusplus
extern "C" {
#endif
int xpic_set_particles(xpic_ctx* ctx, int sort, const xpic_set_particles_params* params, int64_t n, int64_t particle0,
  int64_t step, int64_t* added, double* energy);
/* ParticlesBuilder::load_coordinate's number_of_particles (src/commands/builders/particles_builder.cpp:16-34), with its
 * truncation to an integer: Np (precise); (max - min) x y z Np / (dx dy dz) (box); pi radius^2 height Np / (dx dy dz)
 * (cylinder); as an extension pi (outer^2 - inner^2) height Np / (dx dy dz) (annulus).  geom as xpic_set_particles_params'.
 * Reads the context's spacings and the sort's Np; touches nothing. */
int xpic_particles_number(xpic_ctx* ctx, int sort, int coordinate, const double geom[7], int64_t* out);
#ifdef __cplusplus
}
#endif
#endif
