// xpic_host.h -- C++ mirror of xpic's Simulation / Particles / Command / Diagnostic interfaces on top of the
// C ABI (include/xpic_hip.h).  Same names, argument meaning and error behaviour as the reference so that the
// backends select like any other `"Simulation"` of the JSON config:
//   interfaces::Simulation   src/interfaces/simulation.h:14-83, simulation.cpp:16-182
//   interfaces::Particles    src/interfaces/particles.h:11-78
//   interfaces::Command      src/interfaces/command.h:14-31
//   interfaces::Diagnostic   src/interfaces/diagnostic.h
//   Configuration            src/utils/configuration.h, configuration.cpp:19-130
//   Builder::parse_value     src/interfaces/builder.cpp:54-81
// PetscErrorCode is `int` here (0 = success); PetscCall is the early-return macro XCALL.
#pragma once

#include <fstream>
#include <functional>
#include <memory>
#include <string>
#include <vector>

#include "../../include/xpic_hip.h"
#include "json.h"

using PetscErrorCode = int;
using PetscInt = int;
using PetscReal = double;

#define XCALL(expr)            \
  do {                         \
    int xrc_ = (expr);         \
    if (xrc_ != 0) return xrc_; \
  } while (0)

// ---- global geometry, as src/constants.h:10-28
extern PetscReal dx, dy, dz, dt;
extern PetscReal geom_x, geom_y, geom_z, geom_t;
extern PetscInt geom_nx, geom_ny, geom_nz, geom_nt;
extern PetscInt diagnose_period;
constexpr PetscReal mec2 = 511.0;

struct Vector3R {
  PetscReal data[3] = {0, 0, 0};
  PetscReal& operator[](int i) { return data[i]; }
  const PetscReal& operator[](int i) const { return data[i]; }
  PetscReal squared() const { return data[0] * data[0] + data[1] * data[1] + data[2] * data[2]; }
};

struct Point { // src/interfaces/point.h:7-35
  Vector3R r, p;
};

struct SortParameters { // src/interfaces/sort_parameters.h:7-19
  std::string sort_name;
  PetscInt Np = 1;
  PetscReal n = 0, q = 0, m = 1;
  PetscReal px = 0, py = 0, pz = 0;
  PetscReal Tx = 0, Ty = 0, Tz = 0;
};

class Configuration { // src/utils/configuration.h
public:
  using json_t = xjson::Value;
  static const Configuration& get();
  static void init(const std::string& config_path);
  static void overwrite(json_t&& json);
  static void set_out_dir(const std::string& dir);
  static bool is_loaded_from_backup(); // configuration.cpp:76-86
  std::string config_path;
  json_t json;
  std::string out_dir;

private:
  static Configuration config;
};
#define CONFIG() Configuration::get()

struct World { // src/utils/world.h:11-61 (the DMDA is the device-side grid of the context)
  PetscErrorCode initialize();
  xpic_geometry geom{};
  static void set_geometry(PetscReal gx, PetscReal gy, PetscReal gz, PetscReal gt, PetscReal dx_, PetscReal dy_,
    PetscReal dz_, PetscReal dt_, PetscReal dtp);
};

namespace interfaces {

class Simulation;

struct Builder { // src/interfaces/builder.cpp:22-113
  static Vector3R parse_vector(const Configuration::json_t& info, const std::string& name);
  static PetscReal parse_value(const Configuration::json_t& value);
};

class Particles { // src/interfaces/particles.h:11-78
public:
  Particles(Simulation& simulation, const SortParameters& parameters);
  virtual ~Particles() = default;

  const SortParameters parameters;
  int sort_id = -1; // handle of the species inside the device context

  /// Points pass the local-box test on the device; `is_added` answers immediately from the same FLOOR_STEP test.
  PetscErrorCode add_particle(const Point& point, bool* is_added = nullptr);
  PetscErrorCode flush();          // ships buffered points (xpic_sort_add_particles)
  PetscErrorCode update_cells();   // update_cells_seq / update_cells_mpi
  PetscErrorCode storage(std::vector<Point>& points, std::vector<int>& cell_of); // host mirror on demand
  PetscInt count();

  PetscReal q_m() const { return parameters.q / parameters.m; }
  PetscReal n_Np() const { return parameters.n / parameters.Np; }
  PetscReal qn_Np() const { return parameters.q * parameters.n / parameters.Np; }

protected:
  Simulation& simulation_;
  std::vector<double> pending_;
};

class Command { // src/interfaces/command.h:14-31
public:
  virtual ~Command() = default;
  virtual PetscErrorCode finalize() { return 0; }
  virtual PetscErrorCode execute(PetscInt timestep) = 0;
};

class Diagnostic {
public:
  virtual ~Diagnostic() = default;
  virtual PetscErrorCode finalize() { return 0; }
  virtual PetscErrorCode diagnose(PetscInt timestep) = 0;
};

class Simulation { // src/interfaces/simulation.h:14-83
public:
  Simulation() = default;
  virtual ~Simulation();

  PetscInt start = 0;
  World world;
  xpic_ctx* ctx = nullptr; // plays the role of `DM da` + the owned Vec/Mat/KSP objects

  std::vector<std::shared_ptr<Particles>> particles_;

  PetscErrorCode initialize();
  PetscErrorCode calculate();
  virtual PetscErrorCode finalize();

  /// "E" | "B" | "B0" -> field id of the C ABI (get_named_vector, simulation.cpp:135-143)
  int get_named_vector(const std::string& name) const;
  Particles& get_named_particles(const std::string& name);

  virtual int scheme() const = 0;

protected:
  PetscErrorCode init_particles(); // src/interfaces/simulation.tpp:7-79
  virtual PetscErrorCode initialize_implementation();
  virtual PetscErrorCode timestep_implementation(PetscInt timestep);

  std::vector<std::unique_ptr<Command>> step_presets_;

public:
  const std::vector<std::unique_ptr<Command>>& step_presets() const { return step_presets_; }

protected:
  std::vector<std::unique_ptr<Diagnostic>> diagnostics_;
  friend class ::Configuration;
};

}  // namespace interfaces

namespace basic {
class Simulation final : public interfaces::Simulation { // src/impls/basic/simulation.h
public:
  int scheme() const override { return XPIC_BASIC; }
};
}  // namespace basic

namespace ecsim {
class Simulation : public interfaces::Simulation { // src/impls/ecsim/simulation.h
public:
  int scheme() const override { return XPIC_ECSIM; }
  PetscInt last_ksp_iterations = 0;

protected:
  PetscErrorCode timestep_implementation(PetscInt timestep) override;
};
}  // namespace ecsim

namespace ecsimcorr {
class Simulation final : public ecsim::Simulation { // src/impls/ecsimcorr/simulation.h
public:
  int scheme() const override { return XPIC_ECSIMCORR; }
};
}  // namespace ecsimcorr

namespace electrostatic {
// "Simulation": "electrostatic" (an extension: the reference has no electrostatic scheme; include/xpic_es.h): the XPIC_ES
// context behind the usual Particles, Presets and energy tables.  B is the external static field (SetMagneticField with
// "field": "B"; the scheme holds no B0, so backups hold E and B); there is no current, so no charge_conservation.txt.  The
// "GaussLaw" key: at_start is honoured (the electrostatic start), "every" > 0 is refused -- the step solves Gauss's law
// itself; temporal/gauss_law.txt is written with or without the key, one row per step from the step's own solve.
class Simulation final : public interfaces::Simulation {
public:
  int scheme() const override { return XPIC_ES; }
  PetscInt last_cg_iterations = 0;

protected:
  PetscErrorCode timestep_implementation(PetscInt timestep) override;
};
}  // namespace electrostatic

/// @returns Concrete simulation using `config` specification (src/interfaces/simulation.cpp:160-182).
std::unique_ptr<interfaces::Simulation> build_simulation();

// ---- commands (src/commands/set_particles.cpp, set_magnetic_field.cpp, builders/*)
using CoordinateGenerator = std::function<Vector3R()>;
using MomentumGenerator = std::function<Vector3R(const Vector3R&)>;

class SetParticles : public interfaces::Command {
public:
  SetParticles(interfaces::Particles& particles, PetscInt number_of_particles, CoordinateGenerator gc,
    MomentumGenerator gm);
  PetscErrorCode execute(PetscInt t) override;
  PetscInt added_particles = 0;
  PetscReal added_energy = 0;

private:
  interfaces::Particles& particles_;
  PetscInt number_of_particles_;
  CoordinateGenerator generate_coordinate_;
  MomentumGenerator generate_momentum_;
};

// EXTENSION (not reference behaviour): a SetParticles entry with "device": true is drawn on the device by
// xpic_set_particles from this build's counter-based stream ("seed", default 0) instead of std::mt19937 on the host;
// the count is the builder's.  Without the key the entry takes the class above, as it always has.
class SetParticlesDevice : public interfaces::Command {
public:
  SetParticlesDevice(interfaces::Simulation& sim, interfaces::Particles& particles, int64_t number_of_particles,
    const xpic_set_particles_params& params);
  PetscErrorCode execute(PetscInt t) override;
  int64_t added_particles = 0;
  PetscReal added_energy = 0;

private:
  interfaces::Simulation& sim_;
  interfaces::Particles& particles_;
  int64_t number_of_particles_;
  xpic_set_particles_params params_;
};

class SetMagneticField : public interfaces::Command {
public:
  SetMagneticField(interfaces::Simulation& sim, int field, int field_axpy, const Vector3R& uniform_value);
  // SetCoilsField (set_magnetic_field.cpp:38-150): coils3 = {z0, R, I} per coil, added to the field
  SetMagneticField(interfaces::Simulation& sim, int field, int field_axpy, std::vector<double> coils3);
  PetscErrorCode execute(PetscInt t) override;

private:
  interfaces::Simulation& sim_;
  int field_, field_axpy_;
  Vector3R value_;
  std::vector<double> coils_; // empty: SetUniformField
};

// Builder::load_geometry (src/interfaces/builder.cpp:83-113) of a "BoxGeometry" / "CylinderGeometry" entry ->
// enum xpic_vgeometry and the geom[7] layout of the C ABI
int geometry_kind(const std::string& name); // "BoxGeometry" / "CylinderGeometry"
void load_geometry(const Configuration::json_t& info, int kind, double geom[7]);

// src/commands/remove_particles.cpp:11-40 (xpic_remove_particles)
class RemoveParticles : public interfaces::Command {
public:
  RemoveParticles(interfaces::Simulation& sim, interfaces::Particles& particles, int kind, const double geom[7]);
  PetscErrorCode execute(PetscInt t) override;
  const std::string& get_particles_name() const { return particles_.parameters.sort_name; }
  PetscReal get_removed_energy() const { return removed_energy_; }

private:
  interfaces::Simulation& sim_;
  interfaces::Particles& particles_;
  int kind_;
  double geom_[7];
  PetscReal removed_energy_ = 0;
};

// src/commands/fields_damping.cpp:15-111 (xpic_fields_damping)
class FieldsDamping : public interfaces::Command {
public:
  FieldsDamping(interfaces::Simulation& sim, int E, int B, int B0, int kind, const double geom[7], PetscReal coefficient);
  PetscErrorCode execute(PetscInt t) override;
  PetscReal get_damped_energy() const { return damped_energy_; }

private:
  interfaces::Simulation& sim_;
  int E_, B_, B0_, kind_;
  double geom_[7];
  PetscReal coefficient_, damped_energy_ = 0;
};

// InjectParticlesBuilder::build (src/commands/builders/inject_particles_builder.cpp:11-71): the window and the pairs per step
struct InjectionSchedule {
  PetscInt start = 0, end = 1, per_step = 0;
};
InjectionSchedule injection_schedule(const Configuration::json_t& info, PetscInt ionized_Np);

// src/commands/inject_particles.cpp:26-63 (xpic_inject_particles: the pairs are drawn on the device from a stream keyed by
// (seed, step, pair), not from the host's mt19937)
class InjectParticles : public interfaces::Command {
public:
  InjectParticles(interfaces::Simulation& sim, interfaces::Particles& ionized, interfaces::Particles& ejected,
    const InjectionSchedule& schedule, const xpic_inject_params& params);
  PetscErrorCode execute(PetscInt t) override;
  const std::string& get_ionized_name() const { return ionized_.parameters.sort_name; }
  const std::string& get_ejected_name() const { return ejected_.parameters.sort_name; }
  PetscReal get_ionized_energy() const { return energy_i_; }
  PetscReal get_ejected_energy() const { return energy_e_; }

private:
  interfaces::Simulation& sim_;
  interfaces::Particles &ionized_, &ejected_;
  InjectionSchedule schedule_;
  xpic_inject_params params_;
  PetscReal energy_i_ = 0, energy_e_ = 0;
};

// "BinaryCollisions": Takizuka-Abe binary collisions between the records of one cell (xpic_collide).  AN EXTENSION of the
// reference's JSON surface, which has no collision command: {"command": "BinaryCollisions", "particles": [a, b] or a,
// "strength": S, "seed": ...}; one name (or the same name twice) collides a sort with itself.  "seed" is a JSON number
// (the reader holds numbers as doubles: whole values up to 2^53; a larger or fractional one is refused); without it the
// seed is the command's place in its list, so two commands draw different streams and reordering the list changes them:
// give seeds to keep the streams of a run whose presets are rearranged.  "weighted": true (optional, default false) calls
// xpic_collide_weighted (Nanbu-Yonemura), which accepts two sorts of different weight n / Np; without it the command is
// xpic_collide and refuses such a pair.
class BinaryCollisions : public interfaces::Command {
public:
  BinaryCollisions(interfaces::Simulation& sim, interfaces::Particles& a, interfaces::Particles& b,
    const xpic_collision_params& params, bool weighted);
  PetscErrorCode execute(PetscInt t) override;

private:
  interfaces::Simulation& sim_;
  interfaces::Particles &a_, &b_;
  xpic_collision_params params_;
  bool weighted_;
};

PetscErrorCode build_commands(interfaces::Simulation& simulation, const std::string& name,
  std::vector<std::unique_ptr<interfaces::Command>>& result);

// ---- diagnostics (src/diagnostics/utils/table_diagnostic.cpp, src/diagnostics/energy.cpp)
class TableDiagnostic : public interfaces::Diagnostic {
public:
  explicit TableDiagnostic(const std::string& filename);
  PetscErrorCode diagnose(PetscInt t) override;
  PetscErrorCode finalize() override { file_.close(); return 0; }
  virtual PetscErrorCode initialize() { return 0; }
  virtual PetscErrorCode add_columns(PetscInt /* t */) { return 0; }
  void add(PetscInt w, std::string title, const char* printf_fmt, double value, PetscInt pos = -1);
  void add_int(PetscInt w, std::string title, long value);

protected:
  void write_formatted(const std::vector<std::string>& container);
  std::string filename_;
  std::ofstream file_;
  std::vector<std::string> titles_, values_;
  bool initialized_ = false;
};

class Energy : public interfaces::Diagnostic {
public:
  explicit Energy(interfaces::Simulation& simulation);
  PetscErrorCode diagnose(PetscInt t) override;

protected:
  PetscErrorCode calculate();
  interfaces::Simulation& simulation;
  TableDiagnostic energy, energy_cons;
  PetscReal E = 0, E0 = 0, B = 0, B0 = 0, std_E = 0, std_B = 0;
  std::vector<PetscReal> K, K0, std_K;
};

class ChargeConservation : public TableDiagnostic { // src/diagnostics/charge_conservation.cpp:100-171
public:
  explicit ChargeConservation(interfaces::Simulation& simulation);
  PetscErrorCode initialize() override;
  PetscErrorCode add_columns(PetscInt t) override;

private:
  interfaces::Simulation& simulation;
};

// The optional top-level "GaussLaw" object (an extension: the reference has no Gauss-law cleaner; include/xpic_gauss.h):
//   {"at_start": bool, "every": int, "rtol": 1e-10, "atol": 0, "maxit": 10000, "background": "neutralize", "solver": "cg"}
// solver: "cg" or "direct" (include/xpic_poisson.h: the Hartley-transform solve, whose iterations count its applications), for
// the start clean, the riding clean and an electrostatic simulation's step alike; without the key nothing is set.
// at_start: the run's initial E is cleaned once the presets have loaded the particles (the electrostatic start); every k > 0:
// xpic_step cleans E on every k-th step.  "background": "neutralize" (the default, and the only kind) names what the clean
// does with a net charge: its mean is taken out as a uniform neutralising background and reported.  One row per diagnosed
// step in temporal/gauss_law.txt: |res|_2 before and after, the mean taken out, the iterations; on a step without a clean
// both norms are the residual as it stands and the iterations are 0.
class GaussLaw : public TableDiagnostic {
public:
  GaussLaw(interfaces::Simulation& simulation, const Configuration::json_t& info);
  explicit GaussLaw(interfaces::Simulation& simulation); // no key (an electrostatic run's table): the defaults below
  PetscErrorCode start(); // after the presets, before the first diagnose
  PetscErrorCode add_columns(PetscInt t) override;

private:
  interfaces::Simulation& simulation;
  bool at_start_ = false;
  int every_ = 0, maxit_ = 10000, solver_ = -1;
  double rtol_ = 1e-10, atol_ = 0.0, cleans_seen_ = 0.0;
};

class MomentumConservation : public TableDiagnostic { // src/diagnostics/momentum_conservation.cpp:7-131
public:
  explicit MomentumConservation(interfaces::Simulation& simulation);
  PetscErrorCode initialize() override;
  PetscErrorCode add_columns(PetscInt t) override;

private:
  PetscErrorCode calculate(); // P1, QE of every sort: the sums stay on the device (xpic_momentum)
  interfaces::Simulation& simulation;
  std::vector<Vector3R> P0, P1, QE;
};

PetscErrorCode build_diagnostics(interfaces::Simulation& simulation,
  std::vector<std::unique_ptr<interfaces::Diagnostic>>& result); // diagnostic_builder.cpp:16-75

// ---- float32 dumps (src/diagnostics/field_view.cpp, src/utils/mpi_binary_file.cpp:95-108): one file
// <out_dir>/<format_time(t)> per diagnose period, the region's values in C order [z][y][x][c] as float32
class FieldView : public interfaces::Diagnostic {
public:
  struct Region { // field_view.h:15-20, axes in x, y, z, component order
    PetscInt dim = 4, dof = 3;
    PetscInt start[4] = {0, 0, 0, 0};
    PetscInt size[4] = {0, 0, 0, 3};
  };
  FieldView(const std::string& out_dir, interfaces::Simulation& simulation, int field, const Region& region);
  PetscErrorCode diagnose(PetscInt t) override;
  static std::string format_time(PetscInt t); // src/interfaces/diagnostic.cpp:21-25

protected:
  virtual PetscErrorCode fetch(std::vector<double>& data); // the whole local array, [z][y][x][dof]
  interfaces::Simulation& simulation;
  std::string out_dir_;
  int field_;
  Region region_;
};

class DistributionMoment final : public FieldView { // src/diagnostics/distribution_moment.cpp, all six moments
public:
  // kind: enum xpic_moment_kind; the deposit follows the region rule of the reference (xpic_moment)
  DistributionMoment(const std::string& out_dir, interfaces::Simulation& simulation, interfaces::Particles& particles,
    int kind, const Region& region);

protected:
  PetscErrorCode fetch(std::vector<double>& data) override;
  interfaces::Particles& particles_;
  int kind_;
};

// src/diagnostics/velocity_distribution.cpp: <out_dir>/<time> = float32 [vsize_y][vsize_x] every diagnose_period steps
class VelocityDistribution final : public interfaces::Diagnostic {
public:
  VelocityDistribution(const std::string& out_dir, interfaces::Simulation& simulation, interfaces::Particles& particles,
    int projector, int geometry, const double geom[7], const double vreg[6]);
  PetscErrorCode diagnose(PetscInt t) override;

private:
  interfaces::Simulation& simulation;
  interfaces::Particles& particles_;
  std::string out_dir_;
  int projector_, geometry_;
  double geom_[7], vreg_[6];
};

// EXTENSION (not reference behaviour): "TracedParticles", test particles that ride along with the run as a tracer set
// (include/xpic_tracers.h).  Keys: "kind" ("full_orbit" | "drift_kinetic"), "scheme" (a full-orbit id, default "B1B"), "qm",
// "mp" (drift kinetic), "dt" (default: the run's), "points": SetParticles-style entries {"coordinate": {"name":
// "PreciseCoordinate", "value": xyz}, "momentum": {"name": "PreciseMomentum", "value": xyz}} (drift kinetic: the value is
// {p_parallel, p_perp, mu_p}), optional "region" (a geometry as RemoveParticles'), "sample_every" (steps, default 1),
// "diagnose_period" (default: the geometry's), "name" (a suffix of the directory).  A guiding-centre set takes grad |B| of
// the run's B by XPIC_GRADB_AUTO.  The set is created and attached when the diagnostics are built; every diagnose_period the
// sample rows held are drained into <out_dir>/traced_particles[_name]/<time> as raw float64 [rows][n][6].  The class
// exists only where the key is present.
// Optional "moments": a list of {"moment" (a DistributionMoment name), "q", "m", optional "weight" (default 1), "every"
// (steps, default 1) and "region" (as FieldView's)}: each is a map of the set (include/xpic_tracer_moments.h).  Every
// diagnose_period the map's time average, out / deposits, is written as float32 to
// <out_dir>/traced_particles[_name]/<moment>/<time> in DistributionMoment's file layout (the region's values
// [z][y][x][c]) and the map is reset; a period without a deposit (the call at `start`) writes no file.  An entry without
// the key runs and writes as it did before the key existed.
class TracedParticles final : public interfaces::Diagnostic {
public:
  struct Moment {
    int map;
    FieldView::Region region;
    std::string dir;
  };
  TracedParticles(const std::string& out_dir, interfaces::Simulation& simulation, int set, int64_t n, int64_t capacity,
    PetscInt period, std::vector<Moment> moments = {});
  PetscErrorCode diagnose(PetscInt t) override;

private:
  interfaces::Simulation& simulation;
  std::string out_dir_;
  int set_;
  int64_t n_, capacity_;
  PetscInt period_;
  std::vector<Moment> moments_;
};

// EXTENSION (not reference behaviour): "FieldLines", the lines of a field of the run through given points, traced on the
// device (include/xpic_field_lines.h).  Keys: "field" ("E" | "B" | "B0"; E takes the electric stagger), "points": entries
// {"coordinate": {"name": "PreciseCoordinate", "value": xyz}} as "TracedParticles" takes them (a "momentum" is not read),
// "h", "max_steps", optional "region" (a geometry as RemoveParticles'), "f_floor" (default 0), "diagnose_period" (default:
// the geometry's), "name" (a suffix of the directory).  Every diagnose_period the lines are traced both ways on the field
// as it stands and <out_dir>/field_lines[_name]/<time> is written as raw float64 [n][2][10]: end x, end y, end z, length,
// volume, fmin, smin, fmax, steps, code.  The class exists only where the key is present.
class FieldLines final : public interfaces::Diagnostic {
public:
  FieldLines(const std::string& out_dir, interfaces::Simulation& simulation, int field, std::vector<double> seeds,
    const xpic_line_params& params, bool open, const xpic_trace_region& region, PetscInt period);
  PetscErrorCode diagnose(PetscInt t) override;

private:
  interfaces::Simulation& simulation;
  std::string out_dir_;
  int field_;
  std::vector<double> seeds_;
  xpic_line_params params_;
  bool open_;
  xpic_trace_region region_;
  PetscInt period_;
};

// EXTENSION (not reference behaviour): "FieldSpectrum", the spectrum of a field component or of the charge density on the
// device (include/xpic_spectrum.h).  Keys: "field" ("E" | "B" | "B0" | "rho"), "comp" (0, 1, 2; not read for "rho"), optional
// "modes" (a list of signed [m_x, m_y, m_z]), optional "dk" and "nshell" (shells of |k| with the edges dk * j, j = 0 .. nshell),
// "diagnose_period" (default: the geometry's), "name" (a suffix of the directory and of the table).  Every diagnose_period
// <out_dir>/field_spectrum[_name]/<time> is written as raw float64: axis_x[nx], axis_y[ny], axis_z[nz], then shell[nshell];
// with "modes", a row "t Re Im Re Im .." (%.17e) is appended to temporal/field_modes[_name].txt.  The class exists only where
// the key is present.
class FieldSpectrum final : public interfaces::Diagnostic {
public:
  FieldSpectrum(const std::string& out_dir, const std::string& table, interfaces::Simulation& simulation, int source, int comp,
    std::vector<int32_t> modes, std::vector<double> edges2, PetscInt period);
  PetscErrorCode diagnose(PetscInt t) override;

private:
  interfaces::Simulation& simulation;
  std::string out_dir_, table_;
  int source_, comp_;
  std::vector<int32_t> modes_;
  std::vector<double> edges2_;
  PetscInt period_;
  bool started_ = false;
};

// ---- restart files (src/diagnostics/simulation_backup.cpp:30-160): <out_dir>/<t>/{E,B,B0} as PETSc binary Vecs
// (big endian: int32 VEC_FILE_CLASSID = 1211214, int32 n, n doubles in natural [z][y][x][c] order), particles as
// <sort_name> = raw big-endian doubles {r, p} per particle and <sort_name>.numparts = one big-endian int32
class SimulationBackup final : public interfaces::Diagnostic, public interfaces::Command {
public:
  SimulationBackup(const std::string& out_dir, PetscInt diagnose_period, interfaces::Simulation& simulation);
  PetscErrorCode diagnose(PetscInt t) override { return save(t); }
  PetscErrorCode execute(PetscInt t) override { return load(t); }
  PetscErrorCode finalize() override { return 0; }
  PetscErrorCode save(PetscInt t);
  PetscErrorCode load(PetscInt t);
  static constexpr PetscInt num_periods_being_kept = 2;

private:
  std::string out_dir_;
  PetscInt diagnose_period_;
  interfaces::Simulation& simulation;
};
