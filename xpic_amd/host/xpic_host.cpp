// xpic_host.cpp -- see xpic_host.h.  Host logic only; every grid/particle operation goes through the C ABI.
#include "xpic_host.h"

#include <sys/stat.h>

#include <cstdint>
#include <cstring>
#include <filesystem>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <iostream>
#include <map>
#include <random>
#include <sstream>
#include <stdexcept>

PetscReal dx = 0, dy = 0, dz = 0, dt = 0;
PetscReal geom_x = 0, geom_y = 0, geom_z = 0, geom_t = 0;
PetscInt geom_nx = 0, geom_ny = 0, geom_nz = 0, geom_nt = 0;
PetscInt diagnose_period = 0;

#define LOG(msg) (std::cout << msg << "\n")
#define ROUND_STEP(s, ds) static_cast<PetscInt>(std::round((s) / (ds))) /* src/utils/utils.h:77 */
#define FLOOR_STEP(s, ds) static_cast<PetscInt>(std::floor((s) / (ds))) /* :78 */

static int check(interfaces::Simulation* sim, int rc, const char* what)
{
  (void)sim;
  if (rc != 0) std::cerr << "xpic_hip error in " << what << ": " << xpic_last_error() << std::endl;
  return rc;
}
#define HIPCALL(expr) XCALL(check(nullptr, (expr), #expr))

static void make_dirs(const std::string& path)
{
  std::string cur;
  for (size_t i = 0; i <= path.size(); ++i) {
    if (i == path.size() || path[i] == '/') {
      if (!cur.empty()) mkdir(cur.c_str(), 0777);
    }
    if (i < path.size()) cur += path[i];
  }
}

// ---- Configuration (src/utils/configuration.cpp:7-24)
Configuration Configuration::config;
const Configuration& Configuration::get() { return config; }
void Configuration::overwrite(json_t&& json)
{
  config.json = std::move(json);
  config.out_dir = config.json.at("OutputDirectory").as_string();
}
void Configuration::init(const std::string& config_path)
{
  std::ifstream file(config_path);
  if (!file) throw std::runtime_error("Cannot open configuration file " + config_path);
  std::stringstream ss;
  ss << file.rdbuf();
  overwrite(xjson::parse(ss.str()));
  config.config_path = config_path;
}
bool Configuration::is_loaded_from_backup()
{
  const json_t* it = config.json.find("SimulationBackup");
  if (!it) return false;
  const json_t* load_it = it->find("load_from");
  return load_it && load_it->type == xjson::Value::Number && load_it->as_double() == std::floor(load_it->as_double());
}
void Configuration::set_out_dir(const std::string& dir) { config.out_dir = dir; }

// ---- World (src/utils/world.cpp:11-112)
/* static */ void World::set_geometry(PetscReal gx, PetscReal gy, PetscReal gz, PetscReal gt, PetscReal dx_,
  PetscReal dy_, PetscReal dz_, PetscReal dt_, PetscReal dtp)
{
  dx = dx_; dy = dy_; dz = dz_; dt = dt_;
  geom_x = gx; geom_y = gy; geom_z = gz; geom_t = gt;
  geom_nx = ROUND_STEP(geom_x, dx);
  geom_ny = ROUND_STEP(geom_y, dy);
  geom_nz = ROUND_STEP(geom_z, dz);
  geom_nt = ROUND_STEP(geom_t, dt);
  diagnose_period = ROUND_STEP(dtp, dt);
}

PetscErrorCode World::initialize()
{
  const Configuration::json_t& geometry = CONFIG().json.at("Geometry");
  // cell sizes first, parse_value() needs them (world.cpp:17-21)
  dx = geometry.at("dx").as_double();
  dy = geometry.at("dy").as_double();
  dz = geometry.at("dz").as_double();
  dt = geometry.at("dt").as_double();
  using interfaces::Builder;
  set_geometry(Builder::parse_value(geometry.at("x")), Builder::parse_value(geometry.at("y")),
    Builder::parse_value(geometry.at("z")), Builder::parse_value(geometry.at("t")), dx, dy, dz, dt,
    Builder::parse_value(geometry.at("diagnose_period")));
  for (const char* b : {"da_boundary_x", "da_boundary_y", "da_boundary_z"})
    if (geometry.at(b).as_string() != "DM_BOUNDARY_PERIODIC")
      throw std::runtime_error("the HIP backends support DM_BOUNDARY_PERIODIC only");
  geom.n[0] = geom_nx; geom.n[1] = geom_ny; geom.n[2] = geom_nz;
  geom.d[0] = dx; geom.d[1] = dy; geom.d[2] = dz;
  geom.dt = dt;
  geom.periodic[0] = geom.periodic[1] = geom.periodic[2] = 1;
  geom.rank = 0; geom.nranks = 1; geom.device = 0;
  return 0;
}

namespace interfaces {

// ---- Builder (src/interfaces/builder.cpp:22-81)
static bool ends_with(const std::string& s, const std::string& suf)
{
  return s.size() >= suf.size() && s.compare(s.size() - suf.size(), suf.size(), suf) == 0;
}

/* static */ PetscReal Builder::parse_value(const Configuration::json_t& value)
{
  if (!value.is_string()) return value.as_double();
  const std::string& str = value.as_string();
  if (str == "geom_x" || str == "geom_nx") return geom_x;
  if (str == "geom_y" || str == "geom_ny") return geom_y;
  if (str == "geom_z" || str == "geom_nz") return geom_z;
  if (ends_with(str, " [dx]")) return std::stod(str.substr(0, str.size() - 5)) * dx;
  if (ends_with(str, " [dy]")) return std::stod(str.substr(0, str.size() - 5)) * dy;
  if (ends_with(str, " [dz]")) return std::stod(str.substr(0, str.size() - 5)) * dz;
  if (ends_with(str, " [dt]")) return std::stod(str.substr(0, str.size() - 5)) * dt;
  if (ends_with(str, " [c/w_pe]") || ends_with(str, " [1/w_pe]")) return std::stod(str.substr(0, str.size() - 9));
  throw std::runtime_error("Unknown string format to convert: " + str);
}

/* static */ Vector3R Builder::parse_vector(const Configuration::json_t& info, const std::string& name)
{
  const Configuration::json_t& value = info.at(name);
  Vector3R result;
  if (value.is_array()) {
    if (value.arr.size() != 3) throw std::runtime_error(name + " vector should be of size 3.");
    for (int i = 0; i < 3; ++i) result[i] = parse_value(value.arr[i]);
    return result;
  }
  if (value.is_string()) {
    const std::string& str = value.as_string();
    if (str == "Geom") { result[0] = geom_x; result[1] = geom_y; result[2] = geom_z; }
    else if (str == "Geom / 2") { result[0] = geom_x / 2; result[1] = geom_y / 2; result[2] = geom_z / 2; }
    return result;
  }
  const PetscReal v = parse_value(value);
  result[0] = result[1] = result[2] = v;
  return result;
}

// ---- Particles
Particles::Particles(Simulation& simulation, const SortParameters& parameters)
  : parameters(parameters), simulation_(simulation)
{
}

PetscErrorCode Particles::add_particle(const Point& point, bool* is_added)
{
  // the same FLOOR_STEP bounds test the device applies (src/interfaces/particles.cpp:50-56)
  const PetscInt vx = FLOOR_STEP(point.r[0], dx), vy = FLOOR_STEP(point.r[1], dy), vz = FLOOR_STEP(point.r[2], dz);
  const bool inside = 0 <= vx && vx < geom_nx && 0 <= vy && vy < geom_ny && 0 <= vz && vz < geom_nz;
  if (!inside) return 0;
  for (int c = 0; c < 3; ++c) pending_.push_back(point.r[c]);
  for (int c = 0; c < 3; ++c) pending_.push_back(point.p[c]);
  if (is_added) *is_added = true;
  return 0;
}

PetscErrorCode Particles::flush()
{
  if (pending_.empty()) return 0;
  int64_t added = 0;
  HIPCALL(xpic_sort_add_particles(simulation_.ctx, sort_id, (int64_t)(pending_.size() / 6), pending_.data(), &added));
  pending_.clear();
  pending_.shrink_to_fit();
  return 0;
}

PetscErrorCode Particles::update_cells()
{
  int64_t n;
  HIPCALL(xpic_update_cells(simulation_.ctx, sort_id, &n));
  return 0;
}

PetscInt Particles::count()
{
  int64_t n = 0;
  xpic_sort_count(simulation_.ctx, sort_id, &n);
  return (PetscInt)n;
}

PetscErrorCode Particles::storage(std::vector<Point>& points, std::vector<int>& cell_of)
{
  const PetscInt n = count();
  std::vector<double> raw((size_t)n * 6);
  cell_of.resize(n);
  HIPCALL(xpic_sort_get_particles(simulation_.ctx, sort_id, raw.data(), cell_of.data()));
  points.resize(n);
  for (PetscInt i = 0; i < n; ++i)
    for (int c = 0; c < 3; ++c) { points[i].r[c] = raw[6 * i + c]; points[i].p[c] = raw[6 * i + 3 + c]; }
  return 0;
}

// ---- Simulation (src/interfaces/simulation.cpp:16-155)
Simulation::~Simulation()
{
  if (ctx) xpic_destroy(ctx);
}

PetscErrorCode Simulation::initialize()
{
  XCALL(world.initialize());
  LOG("Geometric constants for the current setup:");
  LOG("  Nx = " << geom_nx << ", Ny = " << geom_ny << ", Nz = " << geom_nz << ", Nt = " << geom_nt << ", dt = " << dt);
  LOG("Running initialize implementation");
  XCALL(initialize_implementation());

  // the always-on conservation diagnostic (simulation.cpp:39-50)
  diagnostics_.emplace_back(std::make_unique<Energy>(*this));
  // (the electrostatic scheme has no current to take the divergence of)
  if (scheme() != XPIC_ES) diagnostics_.emplace_back(std::make_unique<ChargeConservation>(*this)); // simulation.cpp:52-53
  diagnostics_.emplace_back(std::make_unique<MomentumConservation>(*this)); // simulation.cpp:55-56

  std::vector<std::unique_ptr<Command>> presets;
  XCALL(build_commands(*this, "Presets", presets));
  XCALL(build_commands(*this, "StepPresets", step_presets_));
  XCALL(build_diagnostics(*this, diagnostics_));

  GaussLaw* gauss = nullptr; // (an extension; a config without the key runs as before)
  if (const Configuration::json_t* info = CONFIG().json.find("GaussLaw")) {
    auto diagnostic = std::make_unique<GaussLaw>(*this, *info);
    gauss = diagnostic.get();
    diagnostics_.emplace_back(std::move(diagnostic));
  }
  else if (scheme() == XPIC_ES) { // the step's own solve is tabulated whether the key is there or not
    auto diagnostic = std::make_unique<GaussLaw>(*this);
    gauss = diagnostic.get();
    diagnostics_.emplace_back(std::move(diagnostic));
  }

  LOG("Executing presets");
  for (auto&& preset : presets) XCALL(preset->execute(start));
  if (gauss) XCALL(gauss->start());
  for (auto& diagnostic : diagnostics_) XCALL(diagnostic->diagnose(start));
  return 0;
}

PetscErrorCode Simulation::calculate()
{
  LOG("Running the main simulation cycle");
  for (PetscInt t = start + 1; t <= geom_nt; ++t) {
    for (auto& command : step_presets_) XCALL(command->execute(t));
    XCALL(timestep_implementation(t));
    for (auto& diagnostic : diagnostics_) XCALL(diagnostic->diagnose(t));
  }
  return 0;
}

PetscErrorCode Simulation::finalize()
{
  for (auto& command : step_presets_) XCALL(command->finalize());
  for (auto& diagnostic : diagnostics_) XCALL(diagnostic->finalize());
  if (ctx) {
    HIPCALL(xpic_destroy(ctx));
    ctx = nullptr;
  }
  return 0;
}

int Simulation::get_named_vector(const std::string& name) const
{
  if (name == "E") return XPIC_E;
  if (name == "B") return XPIC_B;
  if (name == "B0") return XPIC_B0;
  throw std::out_of_range("no vector named " + name);
}

Particles& Simulation::get_named_particles(const std::string& name)
{
  for (auto& sort : particles_)
    if (sort->parameters.sort_name == name) return *sort;
  throw std::runtime_error("No particles with name " + name);
}

PetscErrorCode Simulation::initialize_implementation()
{
  HIPCALL(xpic_create(&world.geom, scheme(), &ctx));
  return init_particles();
}

PetscErrorCode Simulation::init_particles()
{
  const Configuration::json_t& json = CONFIG().json;
  const Configuration::json_t* it = json.find("Particles");
  if (!it || it->arr.empty()) return 0;
  // capacity: the SetParticles presets tell how many points each sort will get; leave head-room for migration.  The
  // InjectParticles step presets add their pairs of the run to both of their sorts.
  std::map<std::string, int64_t> injected;
  if (const Configuration::json_t* sp = json.find("StepPresets")) {
    for (auto&& info : sp->arr) {
      if (!info.contains("command") || info.at("command").as_string() != "InjectParticles") continue;
      const std::string ionized = info.at("ionized").as_string(), ejected = info.at("ejected").as_string();
      PetscInt Np = 0;
      for (auto&& pinfo : it->arr)
        if (pinfo.contains("sort_name") && pinfo.at("sort_name").as_string() == ionized) Np = pinfo.at("Np").as_int();
      const InjectionSchedule s = injection_schedule(info, Np);
      const int64_t steps = std::max<int64_t>(0, (int64_t)std::min(s.end, geom_nt) - std::max<PetscInt>(s.start, 1) + 1);
      injected[ionized] += steps * std::max<PetscInt>(s.per_step, 0);
      injected[ejected] += steps * std::max<PetscInt>(s.per_step, 0);
    }
  }
  for (auto&& info : it->arr) {
    if (!info.contains("sort_name")) continue;
    SortParameters p;
    p.sort_name = info.at("sort_name").as_string();
    p.Np = info.at("Np").as_int();
    p.n = info.at("n").as_double();
    p.q = info.at("q").as_double();
    p.m = info.at("m").as_double();
    if (info.contains("T")) p.Tx = p.Ty = p.Tz = info.at("T").as_double();
    else {
      p.Tx = info.at("Tx").as_double();
      p.Ty = info.at("Ty").as_double();
      p.Tz = info.at("Tz").as_double();
    }
    // EXTENSION (not reference behaviour): the reference's init_particles never reads the initial momentum
    // (src/interfaces/simulation.tpp:24-41), although SortParameters has it (sort_parameters.h:13-15) and MaxwellianMomentum
    // adds it (src/utils/particles_load.cpp:59-70): without it the JSON surface cannot express the two counter-streaming
    // beams of a two-stream set-up.  Absent keys leave the reference's behaviour (zero drift) untouched.
    if (info.contains("px")) p.px = info.at("px").as_double();
    if (info.contains("py")) p.py = info.at("py").as_double();
    if (info.contains("pz")) p.pz = info.at("pz").as_double();
    auto sort = std::make_shared<Particles>(*this, p);
    xpic_sort_params sp{p.Np, p.n, p.q, p.m};
    const int64_t cells = (int64_t)geom_nx * geom_ny * geom_nz;
    const int64_t capacity = std::max<int64_t>(cells * p.Np * 5 / 4 + 4096, 1 << 16) + injected[p.sort_name];
    HIPCALL(xpic_add_sort(ctx, &sp, capacity, &sort->sort_id));
    particles_.emplace_back(sort);
    LOG("  " << p.sort_name << " are added");
  }
  return 0;
}

PetscErrorCode Simulation::timestep_implementation(PetscInt /* t */)
{
  int its = 0;
  HIPCALL(xpic_step(ctx, &its));
  return 0;
}

}  // namespace interfaces

PetscErrorCode ecsim::Simulation::timestep_implementation(PetscInt /* t */)
{
  int its = 0;
  HIPCALL(xpic_step(ctx, &its));
  last_ksp_iterations = its;
  LOG("  KSPSolve() has finished, iterations: " << its);
  return 0;
}

PetscErrorCode electrostatic::Simulation::timestep_implementation(PetscInt /* t */)
{
  int its = 0;
  HIPCALL(xpic_step(ctx, &its));
  last_cg_iterations = its;
  LOG("  Poisson CG has finished, iterations: " << its);
  return 0;
}

std::unique_ptr<interfaces::Simulation> build_simulation()
{
  const std::string simulation_str = CONFIG().json.at("Simulation").as_string();
  std::unique_ptr<interfaces::Simulation> simulation;
  if (simulation_str == "basic") simulation = std::make_unique<basic::Simulation>();
  else if (simulation_str == "ecsim") simulation = std::make_unique<ecsim::Simulation>();
  else if (simulation_str == "ecsimcorr") simulation = std::make_unique<ecsimcorr::Simulation>();
  else if (simulation_str == "electrostatic") simulation = std::make_unique<electrostatic::Simulation>();
  else throw std::runtime_error("Unkown simulation is used: " + simulation_str);
  LOG("Simulation is built, scheme " << simulation_str);
  return simulation;
}

// ---- particle loaders (src/utils/random_generator.h:8-35, src/utils/particles_load.cpp:11-76)
static std::mt19937& generator()
{
  static std::mt19937 gen; // RANDOM_SEED false (src/constants.h:5): default seed
  return gen;
}
static PetscReal random_01()
{
  static std::uniform_real_distribution<double> distribution(0.0, 1.0);
  return distribution(generator());
}
static PetscReal temperature_momentum(PetscReal temperature, PetscReal mass)
{
  return std::sqrt(-2.0 * (temperature * mass / mec2) * std::log(random_01()));
}

SetParticles::SetParticles(interfaces::Particles& particles, PetscInt number_of_particles, CoordinateGenerator gc,
  MomentumGenerator gm)
  : particles_(particles), number_of_particles_(number_of_particles), generate_coordinate_(std::move(gc)),
    generate_momentum_(std::move(gm))
{
}

PetscErrorCode SetParticles::execute(PetscInt /* t */) // src/commands/set_particles.cpp:19-43
{
  added_energy = 0.0;
  added_particles = 0;
  const PetscReal m = particles_.parameters.m;
  const PetscReal mpw = particles_.parameters.n / particles_.parameters.Np;
  for (PetscInt p = 0; p < number_of_particles_; ++p) {
    Vector3R coordinate = generate_coordinate_();
    Vector3R momentum = generate_momentum_(coordinate);
    bool is_added = false;
    Point point;
    point.r = coordinate;
    point.p = momentum;
    XCALL(particles_.add_particle(point, &is_added));
    if (is_added) {
      added_energy += 0.5 * (m * momentum.squared()) * mpw; // Energy::get_kinetic
      added_particles++;
    }
  }
  XCALL(particles_.flush());
  LOG("  Particles have been added into \"" << particles_.parameters.sort_name << "\": " << added_particles);
  return 0;
}

SetParticlesDevice::SetParticlesDevice(interfaces::Simulation& sim, interfaces::Particles& particles,
  int64_t number_of_particles, const xpic_set_particles_params& params)
  : sim_(sim), particles_(particles), number_of_particles_(number_of_particles), params_(params)
{
}

PetscErrorCode SetParticlesDevice::execute(PetscInt t)
{
  HIPCALL(xpic_set_particles(sim_.ctx, particles_.sort_id, &params_, std::max<int64_t>(number_of_particles_, 0), 0, t,
    &added_particles, &added_energy));
  char energy[40];
  std::snprintf(energy, sizeof(energy), "%.17g", added_energy);
  LOG("  Particles have been added into \"" << particles_.parameters.sort_name << "\" on the device: " << added_particles);
  LOG("    energy: " << energy);
  return 0;
}

SetMagneticField::SetMagneticField(interfaces::Simulation& sim, int field, int field_axpy, const Vector3R& v)
  : sim_(sim), field_(field), field_axpy_(field_axpy), value_(v)
{
}

PetscErrorCode SetMagneticField::execute(PetscInt /* t */) // src/commands/set_magnetic_field.cpp:12-19, 27-35
{
  if (!coils_.empty()) { // SetCoilsField: += into the field (:38-102)
    HIPCALL(xpic_set_coils_field(sim_.ctx, field_, (int)(coils_.size() / 3), coils_.data()));
    if (field_axpy_ >= 0) HIPCALL(xpic_vec_axpy(sim_.ctx, field_axpy_, 1.0, field_));
    return 0;
  }
  const size_t n = (size_t)geom_nx * geom_ny * geom_nz;
  std::vector<double> v(3 * n);
  for (size_t i = 0; i < n; ++i)
    for (int c = 0; c < 3; ++c) v[3 * i + c] = value_[c]; // VecStrideSet
  HIPCALL(xpic_field_set(sim_.ctx, field_, v.data()));
  if (field_axpy_ >= 0) HIPCALL(xpic_vec_axpy(sim_.ctx, field_axpy_, 1.0, field_));
  return 0;
}

int geometry_kind(const std::string& name)
{
  if (name == "BoxGeometry") return XPIC_GEOM_BOX;
  if (name == "CylinderGeometry") return XPIC_GEOM_CYLINDER;
  throw std::runtime_error("Unknown geometry name " + name);
}

void load_geometry(const Configuration::json_t& info, int kind, double geom[7])
{
  using interfaces::Builder;
  for (int i = 0; i < 7; ++i) geom[i] = 0.0;
  if (kind == XPIC_GEOM_BOX) { // builder.cpp:83-94: the whole box by default
    Vector3R mn, mx;
    mx[0] = geom_x; mx[1] = geom_y; mx[2] = geom_z;
    if (info.contains("min")) mn = Builder::parse_vector(info, "min");
    if (info.contains("max")) mx = Builder::parse_vector(info, "max");
    for (int i = 0; i < 3; ++i) { geom[i] = mn[i]; geom[3 + i] = mx[i]; }
    return;
  }
  Vector3R c; // (:96-113): centred, radius min(geom_x, geom_y) / 2, height geom_z
  c[0] = 0.5 * geom_x; c[1] = 0.5 * geom_y; c[2] = 0.5 * geom_z;
  if (info.contains("center")) c = Builder::parse_vector(info, "center");
  for (int i = 0; i < 3; ++i) geom[i] = c[i];
  geom[3] = info.contains("radius") ? info.at("radius").as_double() : 0.5 * std::min(geom_x, geom_y);
  geom[4] = info.contains("height") ? info.at("height").as_double() : geom_z;
}

SetMagneticField::SetMagneticField(interfaces::Simulation& sim, int field, int field_axpy, std::vector<double> coils3)
  : sim_(sim), field_(field), field_axpy_(field_axpy), coils_(std::move(coils3))
{
}

RemoveParticles::RemoveParticles(interfaces::Simulation& sim, interfaces::Particles& particles, int kind, const double geom[7])
  : sim_(sim), particles_(particles), kind_(kind)
{
  std::copy(geom, geom + 7, geom_);
}

PetscErrorCode RemoveParticles::execute(PetscInt /* t */)
{
  int64_t removed = 0;
  HIPCALL(xpic_remove_particles(sim_.ctx, particles_.sort_id, kind_, geom_, &removed, &removed_energy_));
  LOG("  Particles have been removed from \"" << particles_.parameters.sort_name << "\": " << removed);
  return 0;
}

FieldsDamping::FieldsDamping(interfaces::Simulation& sim, int E, int B, int B0, int kind, const double geom[7],
  PetscReal coefficient)
  : sim_(sim), E_(E), B_(B), B0_(B0), kind_(kind), coefficient_(coefficient)
{
  std::copy(geom, geom + 7, geom_);
}

PetscErrorCode FieldsDamping::execute(PetscInt /* t */)
{
  HIPCALL(xpic_fields_damping(sim_.ctx, E_, B_, B0_, kind_, geom_, coefficient_, &damped_energy_));
  LOG("  Fields are damped, additional energy runoff: " << damped_energy_);
  return 0;
}

// InjectParticlesBuilder::build (inject_particles_builder.cpp:11-71) with load_coordinate's count (particles_builder.cpp:10-38)
InjectionSchedule injection_schedule(const Configuration::json_t& info, PetscInt ionized_Np)
{
  InjectionSchedule s; // t in [0, 1] by default (:21-24)
  if (info.contains("injection_start")) s.start = ROUND_STEP(info.at("injection_start").as_double(), dt);
  if (info.contains("injection_end")) {
    const auto& v = info.at("injection_end");
    if (v.is_string()) { if (v.as_string() == "geom_t") s.end = geom_nt; }
    else s.end = ROUND_STEP(v.as_double(), dt);
  }
  const auto& ci = info.at("coordinate");
  const std::string cname = ci.at("name").as_string();
  const PetscReal frac = ionized_Np / (dx * dy * dz);
  PetscInt number = 0;
  double g[7];
  if (cname == "PreciseCoordinate") number = ionized_Np;
  else if (cname == "CoordinateInBox") {
    load_geometry(ci, XPIC_GEOM_BOX, g);
    number = (PetscInt)(((g[3] - g[0]) * (g[4] - g[1]) * (g[5] - g[2])) * frac);
  }
  else if (cname == "CoordinateInCylinder") {
    load_geometry(ci, XPIC_GEOM_CYLINDER, g);
    number = (PetscInt)(M_PI * (g[3] * g[3]) * g[4] * frac);
  }
  else throw std::runtime_error("Unknown coordinate generator name " + cname);
  PetscInt tau = s.end - s.start;
  if (info.contains("tau")) tau = ROUND_STEP(info.at("tau").as_double(), dt);
  if (tau == 0) throw std::runtime_error("InjectParticles: tau is zero steps (a division by zero in the reference)");
  s.per_step = number / tau;
  if (info.contains("per_step_particles_num")) s.per_step = info.at("per_step_particles_num").as_int();
  return s;
}

InjectParticles::InjectParticles(interfaces::Simulation& sim, interfaces::Particles& ionized, interfaces::Particles& ejected,
  const InjectionSchedule& schedule, const xpic_inject_params& params)
  : sim_(sim), ionized_(ionized), ejected_(ejected), schedule_(schedule), params_(params)
{
}

PetscErrorCode InjectParticles::execute(PetscInt t) // inject_particles.cpp:26-63
{
  energy_i_ = energy_e_ = 0.0;
  if (t < schedule_.start || t > schedule_.end) return 0;
  int64_t added = 0;
  double e2[2] = {0, 0};
  HIPCALL(xpic_inject_particles(sim_.ctx, ionized_.sort_id, ejected_.sort_id, &params_, schedule_.per_step, t, &added, e2));
  energy_i_ = e2[0];
  energy_e_ = e2[1];
  LOG("  Particles have been injected: " << added);
  return 0;
}

BinaryCollisions::BinaryCollisions(interfaces::Simulation& sim, interfaces::Particles& a, interfaces::Particles& b,
  const xpic_collision_params& params, bool weighted)
  : sim_(sim), a_(a), b_(b), params_(params), weighted_(weighted)
{
}

PetscErrorCode BinaryCollisions::execute(PetscInt t) // (an extension: no counterpart in the reference)
{
  double out6[6] = {0, 0, 0, 0, 0, 0};
  if (weighted_) HIPCALL(xpic_collide_weighted(sim_.ctx, a_.sort_id, b_.sort_id, &params_, t, out6));
  else HIPCALL(xpic_collide(sim_.ctx, a_.sort_id, b_.sort_id, &params_, t, out6));
  LOG("  Binary collisions" << (weighted_ ? " (weighted)" : "") << " \"" << a_.parameters.sort_name << "\" - \""
    << b_.parameters.sort_name << "\": " << (long)out6[0] << " pairs, mean sigma^2 " << (out6[0] > 0 ? out6[2] / out6[0] : 0.0)
    << ", " << (long)out6[3] << " above 1");
  if (weighted_) LOG("    heavier-side updates: " << (long)out6[4] << " made, " << (long)out6[5] << " rejected");
  return 0;
}

// a SetParticles entry with "device": true -> xpic_set_particles' parameters and the builder's count
// (xpic_particles_number).  Beside the reference's names it takes CoordinateOnAnnulus {center, inner_r, outer_r, height}
// and AngularMomentum {center}, which the reference's builder does not offer.
static std::unique_ptr<interfaces::Command> build_set_particles_device(interfaces::Simulation& simulation,
  interfaces::Particles& particles, const Configuration::json_t& info)
{
  using interfaces::Builder;
  xpic_set_particles_params p{};
  const auto& ci = info.at("coordinate");
  const std::string cname = ci.at("name").as_string();
  if (cname == "PreciseCoordinate") {
    p.coordinate = XPIC_COORD_PRECISE;
    const Vector3R dot = Builder::parse_vector(ci, "value");
    for (int i = 0; i < 3; ++i) p.geom[i] = dot[i];
  }
  else if (cname == "CoordinateInBox") {
    p.coordinate = XPIC_COORD_IN_BOX;
    load_geometry(ci, XPIC_GEOM_BOX, p.geom);
  }
  else if (cname == "CoordinateInCylinder") {
    p.coordinate = XPIC_COORD_IN_CYLINDER;
    load_geometry(ci, XPIC_GEOM_CYLINDER, p.geom);
  }
  else if (cname == "CoordinateOnAnnulus") {
    p.coordinate = XPIC_COORD_ON_ANNULUS;
    load_geometry(ci, XPIC_GEOM_CYLINDER, p.geom); // (the centre's and the height's defaults)
    p.geom[5] = p.geom[4];
    p.geom[3] = ci.at("inner_r").as_double();
    p.geom[4] = ci.at("outer_r").as_double();
  }
  else throw std::runtime_error("Unknown coordinate generator name " + cname);
  const auto& mi = info.at("momentum");
  const std::string mname = mi.at("name").as_string();
  const SortParameters& sp = particles.parameters;
  const double T[3] = {sp.Tx, sp.Ty, sp.Tz}, drift[3] = {sp.px, sp.py, sp.pz};
  for (int i = 0; i < 3; ++i) { p.T[i] = T[i]; p.value[i] = drift[i]; }
  if (mname == "PreciseMomentum") {
    p.momentum = XPIC_MOMENTUM_PRECISE;
    const Vector3R value = Builder::parse_vector(mi, "value");
    for (int i = 0; i < 3; ++i) p.value[i] = value[i];
  }
  else if (mname == "MaxwellianMomentum") {
    p.momentum = XPIC_MOMENTUM_MAXWELLIAN;
    p.tov = mi.contains("tov") ? mi.at("tov").as_bool() : false;
  }
  else if (mname == "MaxwellCosinePerturbation") {
    p.momentum = XPIC_MOMENTUM_COSINE_PERTURBATION;
    double box[7];
    load_geometry(mi, XPIC_GEOM_BOX, box);
    const Vector3R a = Builder::parse_vector(mi, "amplitude"), m = Builder::parse_vector(mi, "wave_number");
    for (int i = 0; i < 3; ++i) { p.amplitude[i] = a[i]; p.wave_number[i] = m[i]; }
    for (int i = 0; i < 6; ++i) p.box6[i] = box[i];
  }
  else if (mname == "AngularMomentum") {
    p.momentum = XPIC_MOMENTUM_ANGULAR;
    Vector3R c;
    c[0] = 0.5 * geom_x; c[1] = 0.5 * geom_y;
    if (mi.contains("center")) c = Builder::parse_vector(mi, "center");
    for (int i = 0; i < 3; ++i) p.center[i] = c[i];
  }
  else throw std::runtime_error("Unknown coordinate generator name " + mname);
  if (info.contains("seed")) p.seed = (uint64_t)info.at("seed").as_double();
  int64_t number = 0;
  if (xpic_particles_number(simulation.ctx, particles.sort_id, p.coordinate, p.geom, &number) != 0)
    throw std::runtime_error(std::string("SetParticles (device): ") + xpic_last_error());
  return std::make_unique<SetParticlesDevice>(simulation, particles, number, p);
}

// build_commands (src/commands/builders/command_builder.cpp:16-62) with ParticlesBuilder::load_coordinate /
// load_momentum (particles_builder.cpp:9-68) and SetMagneticFieldBuilder (set_magnetic_field_builder.cpp:11-63)
PetscErrorCode build_commands(interfaces::Simulation& simulation, const std::string& name,
  std::vector<std::unique_ptr<interfaces::Command>>& result)
{
  using interfaces::Builder;
  if (name == "Presets" && Configuration::is_loaded_from_backup()) { // command_builder.cpp:24-27
    const auto& info = CONFIG().json.at("SimulationBackup");
    const PetscInt load_from = (PetscInt)info.at("load_from").as_double();
    LOG("Restoring simulation from backup at " << load_from * dt << " [1/w_pe], " << load_from << " [dt]");
    simulation.start = load_from; // simulation_backup_builder.cpp:75-79
    result.emplace_back(std::make_unique<SimulationBackup>(CONFIG().out_dir + "/simulation_backup/", -1, simulation));
    return 0;
  }
  const Configuration::json_t* it = CONFIG().json.find(name);
  if (!it || it->arr.empty()) return 0;
  for (auto&& info : it->arr) {
    if (!info.contains("command")) continue;
    const std::string command = info.at("command").as_string();
    if (command == "SetParticles") {
      auto& particles = simulation.get_named_particles(info.at("particles").as_string());
      const auto& ci = info.at("coordinate");
      const std::string cname = ci.at("name").as_string();
      if (info.contains("device") && info.at("device").as_bool()) {
        result.emplace_back(build_set_particles_device(simulation, particles, info));
        LOG("  SetParticles command (device) is added for \"" << particles.parameters.sort_name << "\"");
        continue;
      }
      const PetscInt Np = particles.parameters.Np;
      const PetscReal frac = Np / (dx * dy * dz);
      PetscInt number_of_particles = 0;
      CoordinateGenerator gc;
      if (cname == "PreciseCoordinate") {
        number_of_particles = Np;
        Vector3R dot = Builder::parse_vector(ci, "value");
        gc = [dot]() { return dot; };
      }
      else if (cname == "CoordinateInBox") {
        Vector3R mn, mx;
        mx[0] = geom_x; mx[1] = geom_y; mx[2] = geom_z; // Builder::load_geometry defaults (builder.cpp:83-94)
        if (ci.contains("min")) mn = Builder::parse_vector(ci, "min");
        if (ci.contains("max")) mx = Builder::parse_vector(ci, "max");
        number_of_particles = ((mx[0] - mn[0]) * (mx[1] - mn[1]) * (mx[2] - mn[2])) * frac; // truncation, :26
        gc = [mn, mx]() {
          Vector3R r;
          r[0] = mn[0] + random_01() * (mx[0] - mn[0]);
          r[1] = mn[1] + random_01() * (mx[1] - mn[1]);
          r[2] = mn[2] + random_01() * (mx[2] - mn[2]);
          return r;
        };
      }
      else if (cname == "CoordinateInCylinder") { // particles_load.cpp:20-30, particles_builder.cpp:31-35
        double g[7];
        load_geometry(ci, XPIC_GEOM_CYLINDER, g);
        number_of_particles = M_PI * (g[3] * g[3]) * g[4] * frac; // truncation
        const Vector3R c{{g[0], g[1], g[2]}};
        const PetscReal R = g[3], h = g[4];
        gc = [c, R, h]() {
          const PetscReal r = R * std::sqrt(random_01());
          const PetscReal phi = 2.0 * M_PI * random_01();
          Vector3R p;
          p[0] = c[0] + r * std::cos(phi);
          p[1] = c[1] + r * std::sin(phi);
          p[2] = c[2] + h * (random_01() - 0.5);
          return p;
        };
      }
      else throw std::runtime_error("Unknown coordinate generator name " + cname);
      MomentumGenerator gm;
      const auto& mi = info.at("momentum");
      const std::string mname = mi.at("name").as_string();
      if (mname == "PreciseMomentum") {
        Vector3R value = Builder::parse_vector(mi, "value");
        gm = [value](const Vector3R&) { return value; };
      }
      else if (mname == "MaxwellianMomentum") {
        bool tov = mi.contains("tov") ? mi.at("tov").as_bool() : false;
        SortParameters params = particles.parameters;
        gm = [params, tov](const Vector3R&) { // particles_load.cpp:57-76; sin(2 pi u) is drawn before sqrt(-2..ln u)
          Vector3R result;
          const PetscReal sx = std::sin(2.0 * M_PI * random_01());
          result[0] = params.px + sx * temperature_momentum(params.Tx, params.m);
          const PetscReal sy = std::sin(2.0 * M_PI * random_01());
          result[1] = params.py + sy * temperature_momentum(params.Ty, params.m);
          const PetscReal sz = std::sin(2.0 * M_PI * random_01());
          result[2] = params.pz + sz * temperature_momentum(params.Tz, params.m);
          if (tov) {
            const PetscReal g = std::sqrt(params.m * params.m + result.squared());
            for (int c = 0; c < 3; ++c) result[c] /= g;
          }
          return result;
        };
      }
      else if (mname == "MaxwellCosinePerturbation") { // particles_load.cpp:78-103, particles_builder.cpp:57-65
        double box[7];
        load_geometry(mi, XPIC_GEOM_BOX, box);
        const Vector3R a = Builder::parse_vector(mi, "amplitude"), m = Builder::parse_vector(mi, "wave_number");
        // (the reference keeps the extents in `static const` locals, so its first generator's box serves all; this
        // one takes its own)
        const Vector3R L{{box[3] - box[0], box[4] - box[1], box[5] - box[2]}};
        SortParameters params = particles.parameters;
        gm = [params, a, m, L](const Vector3R& coordinate) {
          const PetscReal T[3] = {params.Tx, params.Ty, params.Tz};
          Vector3R v;
          for (int c = 0; c < 3; ++c) { // sin(2 pi u) is drawn before sqrt(-2..ln u), as in MaxwellianMomentum above
            const PetscReal s = std::sin(2.0 * M_PI * random_01());
            v[c] = s * temperature_momentum(T[c], params.m);
          }
          const PetscReal g = std::sqrt(params.m * params.m + v.squared());
          for (int c = 0; c < 3; ++c) {
            v[c] /= g;
            const PetscReal v0 = a[c] * sqrt(T[c] / (params.m * mec2));
            v[c] += v0 * std::cos(2.0 * M_PI * m[c] * coordinate[c] / L[c]);
          }
          return v;
        };
      }
      else throw std::runtime_error("Unknown coordinate generator name " + mname);
      result.emplace_back(std::make_unique<SetParticles>(particles, number_of_particles, gc, gm));
      LOG("  SetParticles command is added for \"" << particles.parameters.sort_name << "\"");
    }
    else if (command == "SetMagneticField") {
      const int field = simulation.get_named_vector(info.at("field").as_string());
      int axpy = -1;
      if (info.contains("field_axpy")) axpy = simulation.get_named_vector(info.at("field_axpy").as_string());
      const auto& setter = info.at("setter");
      const std::string sname = setter.at("name").as_string();
      if (sname == "SetUniformField")
        result.emplace_back(std::make_unique<SetMagneticField>(simulation, field, axpy, Builder::parse_vector(setter, "value")));
      else if (sname == "SetCoilsField") { // set_magnetic_field_builder.cpp:45-57
        std::vector<double> coils;
        for (auto&& coil : setter.at("coils").arr) {
          coils.push_back(coil.at("z0").as_double());
          coils.push_back(coil.at("R").as_double());
          coils.push_back(coil.at("I").as_double());
          LOG("    Adding magnetic coil, z0: " << coils[coils.size() - 3] << ", R: " << coils[coils.size() - 2] << ", I: " << coils.back());
        }
        result.emplace_back(std::make_unique<SetMagneticField>(simulation, field, axpy, std::move(coils)));
      }
      else throw std::runtime_error("Unknown setter name " + sname);
    }
    else if (command == "RemoveParticles") { // remove_particles_builder.cpp:11-44
      auto& particles = simulation.get_named_particles(info.at("particles").as_string());
      const auto& geometry = info.at("geometry");
      const int kind = geometry_kind(geometry.at("name").as_string());
      double g[7];
      load_geometry(geometry, kind, g);
      result.emplace_back(std::make_unique<RemoveParticles>(simulation, particles, kind, g));
      LOG("  RemoveParticles command is added for \"" << particles.parameters.sort_name << "\"");
    }
    else if (command == "FieldsDamping") { // fields_damping_builder.cpp:11-51
      const int E = simulation.get_named_vector(info.at("E").as_string());
      const int B = simulation.get_named_vector(info.at("B").as_string());
      const int B0 = simulation.get_named_vector(info.at("B0").as_string());
      const PetscReal coefficient = info.at("damping_coefficient").as_double();
      const auto& geometry = info.at("geometry");
      const int kind = geometry_kind(geometry.at("name").as_string());
      double g[7];
      load_geometry(geometry, kind, g);
      result.emplace_back(std::make_unique<FieldsDamping>(simulation, E, B, B0, kind, g, coefficient));
      LOG("  FieldsDamping command is added");
    }
    else if (command == "InjectParticles") { // inject_particles_builder.cpp:11-71
      auto& ionized = simulation.get_named_particles(info.at("ionized").as_string());
      auto& ejected = simulation.get_named_particles(info.at("ejected").as_string());
      const InjectionSchedule schedule = injection_schedule(info, ionized.parameters.Np);
      xpic_inject_params p{};
      const auto& ci = info.at("coordinate");
      const std::string cname = ci.at("name").as_string();
      if (cname == "PreciseCoordinate") {
        p.coordinate = XPIC_COORD_PRECISE;
        const Vector3R v = Builder::parse_vector(ci, "value");
        for (int i = 0; i < 3; ++i) p.geom[i] = v[i];
      }
      else {
        p.coordinate = cname == "CoordinateInBox" ? XPIC_COORD_IN_BOX : XPIC_COORD_IN_CYLINDER;
        load_geometry(ci, cname == "CoordinateInBox" ? XPIC_GEOM_BOX : XPIC_GEOM_CYLINDER, p.geom);
      }
      interfaces::Particles* sorts[2] = {&ionized, &ejected};
      const char* keys[2] = {"momentum_i", "momentum_e"};
      for (int k = 0; k < 2; ++k) { // ParticlesBuilder::load_momentum (particles_builder.cpp:40-68)
        const auto& mi = info.at(keys[k]);
        const std::string mname = mi.at("name").as_string();
        xpic_momentum_params& m = p.momentum[k];
        if (mname == "PreciseMomentum") {
          m.kind = XPIC_MOMENTUM_PRECISE;
          const Vector3R v = Builder::parse_vector(mi, "value");
          for (int i = 0; i < 3; ++i) m.value[i] = v[i];
        }
        else if (mname == "MaxwellianMomentum") {
          const SortParameters& sp = sorts[k]->parameters;
          m.kind = XPIC_MOMENTUM_MAXWELLIAN;
          m.tov = mi.contains("tov") && mi.at("tov").as_bool() ? 1 : 0;
          m.value[0] = sp.px; m.value[1] = sp.py; m.value[2] = sp.pz;
          m.T[0] = sp.Tx; m.T[1] = sp.Ty; m.T[2] = sp.Tz;
        }
        else throw std::runtime_error("Unknown momentum generator name " + mname);
      }
      p.seed = (uint64_t)result.size(); // the command's place in its list: two injections draw different pairs
      result.emplace_back(std::make_unique<InjectParticles>(simulation, ionized, ejected, schedule, p));
      LOG("  InjectParticles command is added with ionized: \"" << ionized.parameters.sort_name << "\", ejected: \""
        << ejected.parameters.sort_name << "\", " << schedule.per_step << " pairs per step in [" << schedule.start << ", "
        << schedule.end << "]");
    }
    else if (command == "BinaryCollisions") { // an extension of the reference's JSON surface (no collision command there)
      const auto& pi = info.at("particles");
      std::string na, nb;
      if (pi.is_string()) na = nb = pi.as_string();
      else {
        if (pi.arr.empty() || pi.arr.size() > 2) throw std::runtime_error("BinaryCollisions: \"particles\" takes one or two sort names");
        na = pi.arr.front().as_string();
        nb = pi.arr.back().as_string();
      }
      auto& a = simulation.get_named_particles(na);
      auto& b = simulation.get_named_particles(nb);
      xpic_collision_params p{};
      p.strength = info.at("strength").as_double();
      p.dt = info.contains("dt") ? info.at("dt").as_double() : 0.0; // (0: the simulation's dt)
      p.seed = (uint64_t)result.size(); // (the command's place in its list, as InjectParticles' seed)
      if (info.contains("seed")) {
        const double sd = info.at("seed").as_double(); // (the reader's numbers are doubles)
        if (!(sd >= 0.0 && sd <= 9007199254740992.0) || sd != std::floor(sd))
          throw std::runtime_error("BinaryCollisions: \"seed\" must be a whole number in [0, 2^53]");
        p.seed = (uint64_t)sd;
      }
      const bool weighted = info.contains("weighted") && info.at("weighted").as_bool();
      result.emplace_back(std::make_unique<BinaryCollisions>(simulation, a, b, p, weighted));
      LOG("  BinaryCollisions command is added for \"" << na << "\" and \"" << nb << "\", strength " << p.strength
        << (weighted ? ", weighted path (xpic_collide_weighted)" : ", equal-weight path (xpic_collide)"));
    }
    else throw std::runtime_error("Unknown command name " + command);
  }
  return 0;
}

// ---- FieldView / DistributionMoment / SimulationBackup and their builders
/* static */ std::string FieldView::format_time(PetscInt t)
{
  const size_t width = std::to_string(geom_nt).size();
  std::string s = std::to_string(t);
  return s.size() < width ? std::string(width - s.size(), '0') + s : s;
}

FieldView::FieldView(const std::string& out_dir, interfaces::Simulation& simulation, int field, const Region& region)
  : simulation(simulation), out_dir_(out_dir), field_(field), region_(region)
{
}

PetscErrorCode FieldView::fetch(std::vector<double>& data)
{
  data.resize((size_t)geom_nx * geom_ny * geom_nz * 3);
  HIPCALL(xpic_field_get(simulation.ctx, field_, data.data()));
  return 0;
}

PetscErrorCode FieldView::diagnose(PetscInt t)
{
  if (diagnose_period > 0 && t % diagnose_period != 0) return 0;
  std::vector<double> data;
  XCALL(fetch(data));
  const PetscInt dof = region_.dof;
  const PetscInt c0 = dof > 1 ? region_.start[3] : 0, nc = dof > 1 ? region_.size[3] : 1;
  std::vector<float> out;
  out.reserve((size_t)region_.size[0] * region_.size[1] * region_.size[2] * nc);
  for (PetscInt z = region_.start[2]; z < region_.start[2] + region_.size[2]; ++z)
    for (PetscInt y = region_.start[1]; y < region_.start[1] + region_.size[1]; ++y)
      for (PetscInt x = region_.start[0]; x < region_.start[0] + region_.size[0]; ++x)
        for (PetscInt cc = c0; cc < c0 + nc; ++cc)
          out.push_back((float)data[(((size_t)z * geom_ny + y) * geom_nx + x) * dof + cc]); // write_floats: double -> float
  make_dirs(out_dir_);
  std::ofstream f(out_dir_ + "/" + format_time(t), std::ios::binary);
  if (!f) throw std::runtime_error("Cannot open " + out_dir_ + "/" + format_time(t));
  f.write(reinterpret_cast<const char*>(out.data()), (std::streamsize)(out.size() * sizeof(float)));
  return 0;
}

DistributionMoment::DistributionMoment(const std::string& out_dir, interfaces::Simulation& simulation,
  interfaces::Particles& particles, int kind, const Region& region)
  : FieldView(out_dir, simulation, -1, region), particles_(particles), kind_(kind)
{
}

// DistributionMoment::collect (distribution_moment.cpp:157-210): only the region's particles and deposits count
PetscErrorCode DistributionMoment::fetch(std::vector<double>& data)
{
  data.resize((size_t)geom_nx * geom_ny * geom_nz * region_.dof);
  const int region6[6] = {(int)region_.start[0], (int)region_.start[1], (int)region_.start[2], (int)region_.size[0],
    (int)region_.size[1], (int)region_.size[2]};
  HIPCALL(xpic_moment(simulation.ctx, particles_.sort_id, kind_, region6, data.data()));
  return 0;
}

VelocityDistribution::VelocityDistribution(const std::string& out_dir, interfaces::Simulation& simulation,
  interfaces::Particles& particles, int projector, int geometry, const double geom[7], const double vreg[6])
  : simulation(simulation), particles_(particles), out_dir_(out_dir), projector_(projector), geometry_(geometry)
{
  std::copy(geom, geom + 7, geom_);
  std::copy(vreg, vreg + 6, vreg_);
}

// DistributionMoment::diagnose + FieldView::diagnose (velocity_distribution.cpp:96-110): the whole histogram, float32
PetscErrorCode VelocityDistribution::diagnose(PetscInt t)
{
  if (diagnose_period > 0 && t % diagnose_period != 0) return 0;
  int vsize[4]; // vsize_x, vsize_y, vstart_x, vstart_y
  HIPCALL(xpic_velocity_distribution(simulation.ctx, particles_.sort_id, projector_, geometry_, geom_, vreg_, vsize, nullptr));
  std::vector<double> data((size_t)vsize[0] * vsize[1]);
  HIPCALL(xpic_velocity_distribution(simulation.ctx, particles_.sort_id, projector_, geometry_, geom_, vreg_, vsize, data.data()));
  std::vector<float> out(data.begin(), data.end());
  make_dirs(out_dir_);
  std::ofstream f(out_dir_ + "/" + FieldView::format_time(t), std::ios::binary);
  if (!f) throw std::runtime_error("Cannot open " + out_dir_ + "/" + FieldView::format_time(t));
  f.write(reinterpret_cast<const char*>(out.data()), (std::streamsize)(out.size() * sizeof(float)));
  return 0;
}

TracedParticles::TracedParticles(const std::string& out_dir, interfaces::Simulation& simulation, int set, int64_t n,
  int64_t capacity, PetscInt period, std::vector<Moment> moments)
  : simulation(simulation), out_dir_(out_dir), set_(set), n_(n), capacity_(capacity), period_(period),
    moments_(std::move(moments))
{
}

// the rows the set has sampled since the last file, [rows][n][6] float64; no rows (the call at `start`): no file
PetscErrorCode TracedParticles::diagnose(PetscInt t)
{
  if (period_ > 0 && t % period_ != 0) return 0;
  std::vector<double> rows((size_t)capacity_ * n_ * 6);
  int64_t count = 0;
  HIPCALL(xpic_tracers_samples(simulation.ctx, set_, rows.data(), nullptr, &count));
  if (count > 0) {
    make_dirs(out_dir_);
    std::ofstream f(out_dir_ + "/" + FieldView::format_time(t), std::ios::binary);
    if (!f) throw std::runtime_error("Cannot open " + out_dir_ + "/" + FieldView::format_time(t));
    f.write(reinterpret_cast<const char*>(rows.data()), (std::streamsize)((size_t)count * n_ * 6 * sizeof(double)));
  }
  // the maps: the time average since the last file, the region's values [z][y][x][c] as float32; then the map starts anew
  for (const Moment& m : moments_) {
    const PetscInt dof = m.region.dof;
    std::vector<double> data((size_t)geom_nx * geom_ny * geom_nz * dof);
    int64_t info[3] = {0, 0, 0};
    HIPCALL(xpic_tracers_map_get(simulation.ctx, set_, m.map, data.data(), info, 1));
    if (info[0] == 0) continue;
    std::vector<float> out;
    out.reserve((size_t)m.region.size[0] * m.region.size[1] * m.region.size[2] * dof);
    for (PetscInt z = m.region.start[2]; z < m.region.start[2] + m.region.size[2]; ++z)
      for (PetscInt y = m.region.start[1]; y < m.region.start[1] + m.region.size[1]; ++y)
        for (PetscInt x = m.region.start[0]; x < m.region.start[0] + m.region.size[0]; ++x)
          for (PetscInt c = 0; c < dof; ++c)
            out.push_back((float)(data[(((size_t)z * geom_ny + y) * geom_nx + x) * dof + c] / (double)info[0]));
    make_dirs(m.dir);
    std::ofstream f(m.dir + "/" + FieldView::format_time(t), std::ios::binary);
    if (!f) throw std::runtime_error("Cannot open " + m.dir + "/" + FieldView::format_time(t));
    f.write(reinterpret_cast<const char*>(out.data()), (std::streamsize)(out.size() * sizeof(float)));
  }
  return 0;
}

FieldLines::FieldLines(const std::string& out_dir, interfaces::Simulation& simulation, int field, std::vector<double> seeds,
  const xpic_line_params& params, bool open, const xpic_trace_region& region, PetscInt period)
  : simulation(simulation), out_dir_(out_dir), field_(field), seeds_(std::move(seeds)), params_(params), open_(open),
    region_(region), period_(period)
{
}

// the lines through the points on the field as it stands: [n][2][10] float64 (xpic_host.h)
PetscErrorCode FieldLines::diagnose(PetscInt t)
{
  if (period_ > 0 && t % period_ != 0) return 0;
  const size_t n = seeds_.size() / 3;
  std::vector<double> end(6 * n), acc[5];
  for (auto& a : acc) a.resize(2 * n);
  std::vector<int64_t> steps(2 * n);
  std::vector<int32_t> code(2 * n);
  HIPCALL(xpic_field_lines(simulation.ctx, field_, (int64_t)n, seeds_.data(), &params_, open_ ? &region_ : nullptr, 0, end.data(),
    acc[0].data(), acc[1].data(), acc[2].data(), acc[3].data(), acc[4].data(), steps.data(), code.data(), nullptr));
  std::vector<double> rows(20 * n);
  for (size_t q = 0; q < n; ++q)
    for (size_t d = 0; d < 2; ++d) {
      double* row = &rows[(2 * q + d) * 10];
      const size_t slot = d * n + q;
      for (int a = 0; a < 3; ++a) row[a] = end[3 * slot + a];
      for (int k = 0; k < 5; ++k) row[3 + k] = acc[k][slot];
      row[8] = (double)steps[slot];
      row[9] = (double)code[slot];
    }
  make_dirs(out_dir_);
  std::ofstream f(out_dir_ + "/" + FieldView::format_time(t), std::ios::binary);
  if (!f) throw std::runtime_error("Cannot open " + out_dir_ + "/" + FieldView::format_time(t));
  f.write(reinterpret_cast<const char*>(rows.data()), (std::streamsize)(rows.size() * sizeof(double)));
  return 0;
}

FieldSpectrum::FieldSpectrum(const std::string& out_dir, const std::string& table, interfaces::Simulation& simulation, int source,
  int comp, std::vector<int32_t> modes, std::vector<double> edges2, PetscInt period)
  : simulation(simulation), out_dir_(out_dir), table_(table), source_(source), comp_(comp), modes_(std::move(modes)),
    edges2_(std::move(edges2)), period_(period)
{
}

// the reduced spectrum of the source as it stands: axis_x, axis_y, axis_z, shell as raw float64; the modes to the table
PetscErrorCode FieldSpectrum::diagnose(PetscInt t)
{
  if (period_ > 0 && t % period_ != 0) return 0;
  const int nshell = edges2_.empty() ? 0 : (int)edges2_.size() - 1;
  std::vector<double> out((size_t)geom_nx + geom_ny + geom_nz + nshell);
  double* ax = out.data();
  HIPCALL(xpic_spectrum(simulation.ctx, source_, comp_, nullptr, ax, ax + geom_nx, ax + geom_nx + geom_ny, nshell,
    nshell ? edges2_.data() : nullptr, nshell ? ax + geom_nx + geom_ny + geom_nz : nullptr, nullptr, nullptr, nullptr));
  make_dirs(out_dir_);
  std::ofstream f(out_dir_ + "/" + FieldView::format_time(t), std::ios::binary);
  if (!f) throw std::runtime_error("Cannot open " + out_dir_ + "/" + FieldView::format_time(t));
  f.write(reinterpret_cast<const char*>(out.data()), (std::streamsize)(out.size() * sizeof(double)));
  if (modes_.empty()) return 0;
  const int nmodes = (int)(modes_.size() / 3);
  std::vector<double> re_im(2 * (size_t)nmodes);
  HIPCALL(xpic_spectrum_modes(simulation.ctx, source_, comp_, nullptr, nmodes, modes_.data(), re_im.data()));
  make_dirs(CONFIG().out_dir + "/temporal");
  std::ofstream table(table_, started_ ? std::ios::app : std::ios::trunc);
  if (!table) throw std::runtime_error("Cannot open " + table_);
  started_ = true;
  char buf[40];
  table << t;
  for (double v : re_im) {
    std::snprintf(buf, sizeof(buf), " % .17e", v);
    table << buf;
  }
  table << "\n";
  return 0;
}

namespace {

std::unique_ptr<interfaces::Diagnostic> build_field_lines(interfaces::Simulation& simulation, const Configuration::json_t& info)
{
  using interfaces::Builder;
  const std::string field = info.at("field").as_string();
  const int id = simulation.get_named_vector(field);
  std::vector<double> seeds;
  for (auto&& point : info.at("points").arr) {
    const auto& ci = point.at("coordinate");
    if (ci.at("name").as_string() != "PreciseCoordinate") throw std::runtime_error("FieldLines points take PreciseCoordinate");
    const Vector3R r = Builder::parse_vector(ci, "value");
    for (int i = 0; i < 3; ++i) seeds.push_back(r[i]);
  }
  xpic_line_params params{};
  params.h = info.at("h").as_double();
  params.max_steps = info.at("max_steps").as_int();
  params.f_floor = info.contains("f_floor") ? info.at("f_floor").as_double() : 0.0;
  params.stagger = field == "E" ? XPIC_STAGGER_E : XPIC_STAGGER_B;
  params.directions = 3;
  xpic_trace_region region{};
  const bool open = info.contains("region");
  if (open) {
    region.geometry = geometry_kind(info.at("region").at("name").as_string());
    region.compact = XPIC_COMPACT_NEVER;
    load_geometry(info.at("region"), region.geometry, region.geom);
  }
  const PetscInt period = info.contains("diagnose_period") ? ROUND_STEP(Builder::parse_value(info.at("diagnose_period")), dt)
                                                           : diagnose_period;
  const std::string dir = CONFIG().out_dir + "/field_lines" + (info.contains("name") ? "_" + info.at("name").as_string() : "");
  LOG("  field lines diagnostic is added for " << field << ": " << seeds.size() / 3 << " points, period " << period << " [dt]");
  return std::make_unique<FieldLines>(dir, simulation, id, std::move(seeds), params, open, region, period);
}

std::unique_ptr<interfaces::Diagnostic> build_field_spectrum(interfaces::Simulation& simulation, const Configuration::json_t& info)
{
  using interfaces::Builder;
  const std::string field = info.at("field").as_string();
  const int source = field == "rho" ? (int)XPIC_SPECTRUM_RHO : simulation.get_named_vector(field);
  const int comp = field == "rho" ? 0 : info.at("comp").as_int();
  if (comp < 0 || comp > 2) throw std::runtime_error("FieldSpectrum comp should be 0, 1 or 2");
  std::vector<int32_t> modes;
  if (info.contains("modes"))
    for (auto&& m : info.at("modes").arr) {
      if (m.arr.size() != 3) throw std::runtime_error("FieldSpectrum modes are [m_x, m_y, m_z]");
      for (int i = 0; i < 3; ++i) modes.push_back((int32_t)m.arr[i].as_int());
    }
  std::vector<double> edges2;
  if (info.contains("dk") || info.contains("nshell")) {
    const double dk = info.at("dk").as_double();
    const int nshell = info.at("nshell").as_int();
    if (!(dk > 0.0) || nshell < 1 || nshell > XPIC_SPECTRUM_MAX_SHELLS)
      throw std::runtime_error("FieldSpectrum takes dk > 0 and nshell in 1 .. " + std::to_string(XPIC_SPECTRUM_MAX_SHELLS));
    for (int j = 0; j <= nshell; ++j) {
      const double e = dk * (double)j;
      edges2.push_back(e * e);
    }
  }
  const PetscInt period = info.contains("diagnose_period") ? ROUND_STEP(Builder::parse_value(info.at("diagnose_period")), dt)
                                                           : diagnose_period;
  const std::string suffix = info.contains("name") ? "_" + info.at("name").as_string() : "";
  LOG("  field spectrum diagnostic is added for " << field << ": " << modes.size() / 3 << " modes, "
    << (edges2.empty() ? 0 : edges2.size() - 1) << " shells, period " << period << " [dt]");
  return std::make_unique<FieldSpectrum>(CONFIG().out_dir + "/field_spectrum" + suffix,
    CONFIG().out_dir + "/temporal/field_modes" + suffix + ".txt", simulation, source, comp, std::move(modes), std::move(edges2), period);
}

void parse_region(const Configuration::json_t& info, FieldView::Region& region, std::string& suffix, const std::string& name);
void check_region(const FieldView::Region& region, const std::string& name);
int moment_kind(const std::string& moment, int* dof);

std::unique_ptr<interfaces::Diagnostic> build_traced_particles(interfaces::Simulation& simulation,
  const Configuration::json_t& info)
{
  using interfaces::Builder;
  static const char* const schemes[XPIC_FO_NSCHEMES] = {"M1A", "M1B", "MLF", "B1A", "B1B", "BLF", "C1A", "C1B", "CLF", "M2A",
    "M2B", "C2A", "B2B", "EB1A", "EB1B", "EBLF", "EB2B", "CN"}; // enum xpic_fo_scheme
  const std::string kind = info.at("kind").as_string();
  if (kind != "full_orbit" && kind != "drift_kinetic") throw std::runtime_error("Unknown TracedParticles kind " + kind);
  const bool dk = kind == "drift_kinetic";
  const double qm = info.at("qm").as_double(), step = info.contains("dt") ? info.at("dt").as_double() : dt;
  xpic_fo_params fo{qm, step, 1e-7, 1e-7, XPIC_FO_B1B, 30}; // the reference's tolerances and iteration limits
  xpic_dk_params gc{qm, dk ? info.at("mp").as_double() : 1.0, step, 1e-12, 1e-12, 30};
  if (info.contains("scheme")) {
    const std::string name = info.at("scheme").as_string();
    const auto it = std::find_if(std::begin(schemes), std::end(schemes), [&](const char* s) { return name == s; });
    if (it == std::end(schemes)) throw std::runtime_error("Unknown TracedParticles scheme " + name);
    fo.scheme = (int32_t)(it - std::begin(schemes));
  }
  std::vector<double> state;
  for (auto&& point : info.at("points").arr) {
    const auto &ci = point.at("coordinate"), &mi = point.at("momentum");
    if (ci.at("name").as_string() != "PreciseCoordinate" || mi.at("name").as_string() != "PreciseMomentum")
      throw std::runtime_error("TracedParticles points take PreciseCoordinate and PreciseMomentum");
    const Vector3R r = Builder::parse_vector(ci, "value"), p = Builder::parse_vector(mi, "value");
    for (int i = 0; i < 3; ++i) state.push_back(r[i]);
    for (int i = 0; i < 3; ++i) state.push_back(p[i]);
  }
  const int64_t n = (int64_t)(state.size() / 6);
  xpic_trace_region region{};
  const bool open = info.contains("region");
  if (open) {
    region.geometry = geometry_kind(info.at("region").at("name").as_string());
    region.compact = XPIC_COMPACT_AUTO;
    load_geometry(info.at("region"), region.geometry, region.geom);
    region.step0 = simulation.start;
  }
  const PetscInt period = info.contains("diagnose_period") ? ROUND_STEP(Builder::parse_value(info.at("diagnose_period")), dt)
                                                           : diagnose_period;
  const int64_t every = info.contains("sample_every") ? info.at("sample_every").as_int() : 1;
  if (every < 1) throw std::runtime_error("TracedParticles sample_every should be >= 1");
  const int64_t capacity = std::max<PetscInt>(period, 1) / every + 1; // the rows of one period, and the one a drain may find early
  int set = -1;
  const void* params = dk ? (const void*)&gc : (const void*)&fo;
  if (check(nullptr, xpic_tracers_create(simulation.ctx, dk ? XPIC_TRACERS_DRIFT_KINETIC : XPIC_TRACERS_FULL_ORBIT, n, params,
        state.data(), open ? &region : nullptr, XPIC_GRADB_AUTO, every, capacity, &set), "xpic_tracers_create") ||
      check(nullptr, xpic_tracers_attach(simulation.ctx, set, 1), "xpic_tracers_attach"))
    throw std::runtime_error("TracedParticles: the tracer set could not be created");
  const std::string dir = CONFIG().out_dir + "/traced_particles" + (info.contains("name") ? "_" + info.at("name").as_string() : "");
  std::vector<TracedParticles::Moment> moments;
  if (info.contains("moments"))
    for (auto&& mi : info.at("moments").arr) {
      const std::string moment = mi.at("moment").as_string(), what = "TracedParticles " + moment;
      TracedParticles::Moment m;
      int dof = 0;
      const int mkind = moment_kind(moment, &dof);
      if (mkind < 0) throw std::runtime_error("Unknown moment name " + moment + " for TracedParticles");
      m.region.size[0] = geom_nx; m.region.size[1] = geom_ny; m.region.size[2] = geom_nz;
      m.region.dim = dof > 1 ? 4 : 3; m.region.dof = dof; m.region.start[3] = 0; m.region.size[3] = dof;
      std::string suffix;
      if (mi.contains("region")) parse_region(mi.at("region"), m.region, suffix, what);
      check_region(m.region, what);
      const int region6[6] = {(int)m.region.start[0], (int)m.region.start[1], (int)m.region.start[2], (int)m.region.size[0],
        (int)m.region.size[1], (int)m.region.size[2]};
      const int64_t map_every = mi.contains("every") ? mi.at("every").as_int() : 1;
      if (check(nullptr, xpic_tracers_map_create(simulation.ctx, set, mkind, mi.at("q").as_double(), mi.at("m").as_double(),
            mi.contains("weight") ? mi.at("weight").as_double() : 1.0, region6, map_every, &m.map), "xpic_tracers_map_create"))
        throw std::runtime_error("TracedParticles: the map of " + moment + " could not be created");
      m.dir = dir + "/" + moment + (suffix.empty() ? "" : "_" + suffix);
      moments.push_back(m);
    }
  LOG("  traced particles diagnostic is added: " << n << " " << kind << " tracers, period " << period << " [dt]");
  if (!moments.empty()) LOG("    with " << moments.size() << " moment maps");
  return std::make_unique<TracedParticles>(dir, simulation, set, n, capacity, period, std::move(moments));
}

// distribution_moment_builder.cpp:16-23: name -> enum xpic_moment_kind and dof; -1: unknown
int moment_kind(const std::string& moment, int* dof)
{
  static const struct { const char* name; int dof, kind; } known[] = {{"density", 1, XPIC_MOMENT_DENSITY},
    {"current", 3, XPIC_MOMENT_CURRENT}, {"momentum_flux", 6, XPIC_MOMENT_MOMENTUM_FLUX},
    {"momentum_flux_cyl", 6, XPIC_MOMENT_MOMENTUM_FLUX_CYL}, {"momentum_flux_diag", 3, XPIC_MOMENT_MOMENTUM_FLUX_DIAG},
    {"momentum_flux_diag_cyl", 3, XPIC_MOMENT_MOMENTUM_FLUX_DIAG_CYL}};
  const auto k = std::find_if(std::begin(known), std::end(known), [&](const auto& e) { return moment == e.name; });
  if (k == std::end(known)) return -1;
  *dof = k->dof;
  return k->kind;
}

// FieldViewBuilder::parse_region_start_size / parse_res_dir_suffix / check_region (field_view_builder.cpp:60-147)
void parse_plane_position(const Configuration::json_t& info, std::string& plane, PetscReal& position)
{
  plane = info.at("plane").as_string();
  if (plane == "X") position = 0.5 * geom_x;
  else if (plane == "Y") position = 0.5 * geom_y;
  else if (plane == "Z") position = 0.5 * geom_z;
  else throw std::runtime_error("Unknown plane " + plane);
  if (info.contains("position")) position = info.at("position").as_double();
}

void parse_region(const Configuration::json_t& info, FieldView::Region& region, std::string& suffix,
  const std::string& name)
{
  using interfaces::Builder;
  Vector3R start, size;
  size[0] = geom_x; size[1] = geom_y; size[2] = geom_z;
  std::string type = info.contains("type") ? info.at("type").as_string() : "3D";
  if (type != "3D" && type != "2D") throw std::runtime_error("Incorrect type is used for " + name + " .");
  if (info.contains("start")) start = Builder::parse_vector(info, "start");
  if (info.contains("size")) size = Builder::parse_vector(info, "size");
  const PetscReal d[3] = {dx, dy, dz};
  if (type == "2D") {
    std::string plane;
    PetscReal position;
    parse_plane_position(info, plane, position);
    const int dir = plane == "X" ? 0 : (plane == "Y" ? 1 : 2);
    start[dir] = position;
    size[dir] = d[dir];
    char buf[32];
    std::snprintf(buf, sizeof(buf), "plane%s_%04d", plane.c_str(), (int)FLOOR_STEP(position, d[dir]));
    suffix += buf;
  }
  for (int i = 0; i < 3; ++i) {
    region.start[i] = FLOOR_STEP(start[i], d[i]);
    region.size[i] = FLOOR_STEP(size[i], d[i]);
  }
}

void check_region(const FieldView::Region& region, const std::string& name)
{
  const PetscInt n[3] = {geom_nx, geom_ny, geom_nz};
  for (int i = 0; i < 3; ++i)
    if (region.start[i] < 0 || region.start[i] + region.size[i] > n[i])
      throw std::runtime_error("Region is not in global boundaries for " + name + " diagnostic.");
  if (!(region.size[0] > 0 && region.size[1] > 0 && region.size[2] > 0))
    throw std::runtime_error("Sizes are invalid for " + name + " diagnostic.");
}

}  // namespace

PetscErrorCode build_diagnostics(interfaces::Simulation& simulation,
  std::vector<std::unique_ptr<interfaces::Diagnostic>>& result)
{
  using interfaces::Builder;
  LOG("Building diagnostics");
  if (const Configuration::json_t* it = CONFIG().json.find("SimulationBackup"); it && !it->obj.empty()) {
    const PetscReal dp_wp = Builder::parse_value(it->at("diagnose_period"));
    const PetscInt dp = ROUND_STEP(dp_wp, dt);
    LOG("  Simulation backup diagnostic is added, diagnose period: " << dp_wp << " [1/w_pe], " << dp << " [dt]");
    const std::string res_dir = CONFIG().out_dir + "/simulation_backup";
    make_dirs(res_dir);
    if (!CONFIG().config_path.empty()) { // Configuration::save (configuration.cpp:26-36)
      std::error_code ec;
      std::filesystem::copy(CONFIG().config_path, res_dir, std::filesystem::copy_options::overwrite_existing, ec);
    }
    result.emplace_back(std::make_unique<SimulationBackup>(res_dir + "/", dp, simulation));
  }
  const Configuration::json_t* list = CONFIG().json.find("Diagnostics");
  if (!list || list->arr.empty()) return 0;
  for (auto&& info : list->arr) {
    if (!info.contains("diagnostic")) continue;
    const std::string name = info.at("diagnostic").as_string();
    FieldView::Region region;
    region.size[0] = geom_nx; region.size[1] = geom_ny; region.size[2] = geom_nz;
    std::string suffix;
    if (name == "FieldView") {
      const std::string field = info.at("field").as_string();
      region.dim = 4; region.dof = 3; region.start[3] = 0; region.size[3] = 3;
      if (info.contains("region")) parse_region(info.at("region"), region, suffix, field);
      check_region(region, field);
      LOG("  field view diagnostic is added for " << field << ", suffix: " << (suffix.empty() ? "<empty>" : suffix));
      if (!suffix.empty()) suffix = "_" + suffix;
      result.emplace_back(std::make_unique<FieldView>(CONFIG().out_dir + "/" + field + suffix + "/", simulation,
        simulation.get_named_vector(field), region));
    }
    else if (name == "DistributionMoment") {
      const std::string particles = info.at("particles").as_string(), moment = info.at("moment").as_string();
      int mdof = 0;
      const int mkind = moment_kind(moment, &mdof); // distribution_moment_builder.cpp:16-23: name -> dof; here also -> enum xpic_moment_kind
      if (mkind < 0) throw std::runtime_error("Unknown moment name " + moment + " for particles " + particles);
      region.dim = mdof > 1 ? 4 : 3; region.dof = mdof; region.start[3] = 0; region.size[3] = mdof;
      if (info.contains("region")) parse_region(info.at("region"), region, suffix, particles + " " + moment);
      check_region(region, particles + " " + moment);
      LOG("  " << moment << " diagnostic is added for " << particles << ", suffix: " << (suffix.empty() ? "<empty>" : suffix));
      if (!suffix.empty()) suffix = "_" + suffix;
      result.emplace_back(std::make_unique<DistributionMoment>(CONFIG().out_dir + "/" + particles + "/" + moment + suffix,
        simulation, simulation.get_named_particles(particles), mkind, region));
    }
    else if (name == "VelocityDistribution") { // velocity_distribution_builder.cpp:13-115
      const std::string particles = info.at("particles").as_string(), projector = info.at("projector").as_string();
      int proj = -1;
      if (projector == "vx_vy") proj = XPIC_PROJ_VX_VY;
      else if (projector == "vz_vxy") proj = XPIC_PROJ_VZ_VXY;
      else if (projector == "vr_vphi") proj = XPIC_PROJ_VR_VPHI;
      else throw std::runtime_error("Unkown projector name " + projector);
      const auto& geometry = info.at("geometry");
      const int gkind = geometry_kind(geometry.at("name").as_string());
      double geom[7];
      load_geometry(geometry, gkind, geom);
      double vreg[6] = {-1, -1, +1, +1, 0, 0}; // vx_min, vy_min, vx_max, vy_max, dvx, dvy
      const auto& dv = info.at("dv");
      vreg[4] = dv.arr.at(0).as_double();
      vreg[5] = dv.arr.at(1).as_double();
      if (info.contains("vmax")) { vreg[2] = info.at("vmax").arr.at(0).as_double(); vreg[3] = info.at("vmax").arr.at(1).as_double(); }
      if (info.contains("vmin")) { vreg[0] = info.at("vmin").arr.at(0).as_double(); vreg[1] = info.at("vmin").arr.at(1).as_double(); }
      LOG("  " << projector << " velocity distribution diagnostic is added for " << particles);
      result.emplace_back(std::make_unique<VelocityDistribution>(CONFIG().out_dir + "/" + particles + "/" + projector, simulation,
        simulation.get_named_particles(particles), proj, gkind, geom, vreg));
    }
    else if (name == "TracedParticles") result.emplace_back(build_traced_particles(simulation, info));
    else if (name == "FieldLines") result.emplace_back(build_field_lines(simulation, info));
    else if (name == "FieldSpectrum") result.emplace_back(build_field_spectrum(simulation, info));
    else throw std::runtime_error("Unknown diagnostic name " + name +
      " (HIP backends: FieldView, DistributionMoment, VelocityDistribution, TracedParticles, FieldLines, FieldSpectrum)");
  }
  return 0;
}

namespace {

// PETSc binary viewers write big endian (PetscViewerBinaryWrite -> PetscByteSwap on little-endian hosts)
void put_be(std::ofstream& f, const void* src, size_t width, size_t count)
{
  const unsigned char* p = static_cast<const unsigned char*>(src);
  std::vector<unsigned char> buf(width * count);
  for (size_t i = 0; i < count; ++i)
    for (size_t b = 0; b < width; ++b) buf[i * width + b] = p[i * width + (width - 1 - b)];
  f.write(reinterpret_cast<const char*>(buf.data()), (std::streamsize)buf.size());
}

bool get_be(std::ifstream& f, void* dst, size_t width, size_t count)
{
  std::vector<unsigned char> buf(width * count);
  f.read(reinterpret_cast<char*>(buf.data()), (std::streamsize)buf.size());
  if ((size_t)f.gcount() != buf.size()) return false;
  unsigned char* p = static_cast<unsigned char*>(dst);
  for (size_t i = 0; i < count; ++i)
    for (size_t b = 0; b < width; ++b) p[i * width + b] = buf[i * width + (width - 1 - b)];
  return true;
}

constexpr int32_t kVecFileClassId = 1211214; // petscvec.h VEC_FILE_CLASSID
const char* const kBackupFields[3] = {"E", "B", "B0"};

}  // namespace

SimulationBackup::SimulationBackup(const std::string& out_dir, PetscInt diagnose_period, interfaces::Simulation& simulation)
  : out_dir_(out_dir), diagnose_period_(diagnose_period), simulation(simulation)
{
}

PetscErrorCode SimulationBackup::save(PetscInt t)
{
  if (diagnose_period_ <= 0 || t % diagnose_period_ != 0) return 0;
  const std::string dir = out_dir_ + "/" + std::to_string(t);
  make_dirs(dir);
  const size_t n3 = (size_t)geom_nx * geom_ny * geom_nz * 3;
  // the PETSc binary Vec header and the .numparts file carry 32-bit counts (PetscInt without --with-64-bit-indices)
  if (n3 > (size_t)INT32_MAX) throw std::runtime_error("SimulationBackup: the Vec length exceeds the 32-bit PetscInt of the file format");
  std::vector<double> data(n3);
  for (const char* name : kBackupFields) { // save_fields :48-63, VecView of a DMDA vector = natural ordering
    if (simulation.scheme() == XPIC_ES && std::string(name) == "B0") continue; // (the electrostatic scheme holds no B0)
    HIPCALL(xpic_field_get(simulation.ctx, simulation.get_named_vector(name), data.data()));
    std::ofstream f(dir + "/" + name, std::ios::binary);
    const int32_t header[2] = {kVecFileClassId, (int32_t)n3};
    put_be(f, header, 4, 2);
    put_be(f, data.data(), 8, n3);
  }
  for (auto& sort : simulation.particles_) { // save_particles :65-91
    std::vector<Point> points;
    std::vector<int> cells;
    XCALL(sort->storage(points, cells));
    if (points.size() > (size_t)INT32_MAX)
      throw std::runtime_error("SimulationBackup: more particles than the 32-bit .numparts file can hold");
    const int32_t numparts = (int32_t)points.size();
    std::ofstream fn(dir + "/" + sort->parameters.sort_name + ".numparts", std::ios::binary);
    put_be(fn, &numparts, 4, 1);
    std::ofstream fp(dir + "/" + sort->parameters.sort_name, std::ios::binary);
    static_assert(sizeof(Point) == 6 * sizeof(double), "Point is six doubles");
    put_be(fp, points.data(), 8, 6 * points.size());
  }
  std::error_code ec; // save_temporal_diagnostics :94-101
  if (std::filesystem::exists(CONFIG().out_dir + "/temporal"))
    std::filesystem::copy(CONFIG().out_dir + "/temporal", dir + "/temporal",
      std::filesystem::copy_options::overwrite_existing | std::filesystem::copy_options::recursive, ec);
  std::filesystem::remove_all(out_dir_ + "/" + std::to_string(t - num_periods_being_kept * diagnose_period_), ec);
  return 0;
}

PetscErrorCode SimulationBackup::load(PetscInt t)
{
  if (!std::filesystem::exists(out_dir_)) throw std::runtime_error("Cannot load the timestep, no backup directory");
  const std::string dir = out_dir_ + "/" + std::to_string(t);
  const size_t n3 = (size_t)geom_nx * geom_ny * geom_nz * 3;
  std::vector<double> data(n3);
  for (const char* name : kBackupFields) { // load_fields :117-131
    if (simulation.scheme() == XPIC_ES && std::string(name) == "B0") continue;
    std::ifstream f(dir + "/" + name, std::ios::binary);
    int32_t header[2] = {0, 0};
    if (!f || !get_be(f, header, 4, 2) || header[0] != kVecFileClassId || (size_t)header[1] != n3 ||
      !get_be(f, data.data(), 8, n3))
      throw std::runtime_error(std::string("Incorrect field data in backup file ") + dir + "/" + name);
    HIPCALL(xpic_field_set(simulation.ctx, simulation.get_named_vector(name), data.data()));
  }
  for (auto& sort : simulation.particles_) { // load_particles :133-160
    const std::string fname = dir + "/" + sort->parameters.sort_name;
    std::ifstream fn(fname + ".numparts", std::ios::binary);
    int32_t numparts = 0;
    if (!fn || !get_be(fn, &numparts, 4, 1)) throw std::runtime_error("Incorrect number of particles to read is specified");
    std::ifstream fp(fname, std::ios::binary);
    Point point;
    for (int32_t i = 0; i < numparts; ++i) {
      if (!fp || !get_be(fp, &point, 8, 6)) throw std::runtime_error("Point structure consists of 6 PetscReal values");
      XCALL(sort->add_particle(point));
    }
    XCALL(sort->flush());
  }
  std::error_code ec; // load_temporal_diagnostics :162-169
  if (std::filesystem::exists(dir + "/temporal"))
    std::filesystem::copy(dir + "/temporal", CONFIG().out_dir + "/temporal",
      std::filesystem::copy_options::overwrite_existing | std::filesystem::copy_options::recursive, ec);
  LOG("  Simulation is successfully loaded from " << t * dt << " [1/w_pe], " << t << " [dt]");
  return 0;
}

// ---- TableDiagnostic (src/diagnostics/utils/table_diagnostic.cpp:8-59, table_diagnostic.h:19-38)
static std::string pad_left(const std::string& s, int w) // std::format("{:<{}.{}s}")
{
  std::string t = s.substr(0, w);
  t.append(w - t.size(), ' ');
  return t;
}
static std::string pad_center(const std::string& s, int w) // std::format("{:^{}.{}s}")
{
  std::string t = s.substr(0, w);
  const int pad = w - (int)t.size();
  const int left = pad / 2;
  return std::string(left, ' ') + t + std::string(pad - left, ' ');
}

TableDiagnostic::TableDiagnostic(const std::string& filename) : filename_(filename) {}

void TableDiagnostic::add(PetscInt w, std::string title, const char* printf_fmt, double value, PetscInt pos)
{
  char buf[64];
  std::snprintf(buf, sizeof(buf), printf_fmt, value);
  title = pad_left(title, w);
  std::string fvalue = pad_center(buf, w);
  if (pos >= 0) {
    titles_.insert(titles_.begin() + pos, title);
    values_.insert(values_.begin() + pos, fvalue);
  }
  else {
    titles_.push_back(title);
    values_.push_back(fvalue);
  }
}

void TableDiagnostic::add_int(PetscInt w, std::string title, long value)
{
  titles_.push_back(pad_left(title, w));
  values_.push_back(pad_center(std::to_string(value), w));
}

void TableDiagnostic::write_formatted(const std::vector<std::string>& container)
{
  for (size_t i = 0; i + 1 < container.size(); ++i) file_ << container[i] << "  ";
  std::string last = container.back();
  while (!last.empty() && last.back() == ' ') last.pop_back();
  file_ << last << "\n";
}

PetscErrorCode TableDiagnostic::diagnose(PetscInt t)
{
  if (!file_.is_open()) {
    const size_t slash = filename_.rfind('/');
    if (slash != std::string::npos) make_dirs(filename_.substr(0, slash));
    file_.open(filename_, t == 0 ? std::ios::out : std::ios::app); // a run restored from a backup appends
    if (!file_) throw std::runtime_error("Cannot open " + filename_);
  }
  if (!initialized_) { // t == 0, or the first step of a run restored from a backup
    XCALL(initialize());
    initialized_ = true;
  }
  XCALL(add_columns(t));
  if (!values_.empty()) {
    if (t == 0) write_formatted(titles_);
    write_formatted(values_);
    titles_.clear();
    values_.clear();
  }
  file_.flush(); // every row (the reference flushes per diagnose period): a backup taken this step copies whole tables
  return 0;
}

// ---- ChargeConservation: the densities, the divergence and both norms stay on the device
ChargeConservation::ChargeConservation(interfaces::Simulation& simulation)
  : TableDiagnostic(CONFIG().out_dir + "/temporal/charge_conservation.txt"), simulation(simulation)
{
}

PetscErrorCode ChargeConservation::initialize()
{
  HIPCALL(xpic_charge_collect(simulation.ctx));
  return 0;
}

PetscErrorCode ChargeConservation::add_columns(PetscInt t)
{
  auto& particles = simulation.particles_;
  std::vector<double> norm(2 * particles.size() + 2);
  HIPCALL(xpic_charge_columns(simulation.ctx, norm.data()));
  add_int(6, "Time", t);
  for (size_t i = 0; i < particles.size(); ++i) {
    add(13, "N1dQ_" + particles[i]->parameters.sort_name, "% .6e", norm[2 * i]);
    add(13, "N2dQ_" + particles[i]->parameters.sort_name, "% .6e", norm[2 * i + 1]);
  }
  add(13, "N1dQ_tot", "% .6e", norm[2 * particles.size()]);
  add(13, "N2dQ_tot", "% .6e", norm[2 * particles.size() + 1]);
  return 0;
}

// ---- GaussLaw (an extension: no counterpart in the reference): the start clean, the clean that rides with the step, one table
GaussLaw::GaussLaw(interfaces::Simulation& simulation, const Configuration::json_t& info)
  : TableDiagnostic(CONFIG().out_dir + "/temporal/gauss_law.txt"), simulation(simulation)
{
  if (info.contains("at_start")) at_start_ = info.at("at_start").as_bool();
  if (info.contains("every")) every_ = info.at("every").as_int();
  if (info.contains("rtol")) rtol_ = info.at("rtol").as_double();
  if (info.contains("atol")) atol_ = info.at("atol").as_double();
  if (info.contains("maxit")) maxit_ = info.at("maxit").as_int();
  if (info.contains("solver")) {
    const std::string solver = info.at("solver").as_string();
    if (solver != "cg" && solver != "direct") throw std::runtime_error("GaussLaw: \"solver\" is \"cg\" or \"direct\"");
    solver_ = solver == "direct" ? XPIC_POISSON_DIRECT : XPIC_POISSON_CG;
  }
  if (info.contains("background") && info.at("background").as_string() != "neutralize")
    throw std::runtime_error("GaussLaw: \"background\" is \"neutralize\" or absent");
  if (every_ < 0) throw std::runtime_error("GaussLaw: \"every\" must be >= 0");
  if (every_ > 0 && simulation.scheme() == XPIC_ES)
    throw std::runtime_error("GaussLaw: \"every\" is refused on an electrostatic simulation: its step solves Gauss's law itself");
  LOG("  GaussLaw is added: at_start " << at_start_ << ", every " << every_ << ", rtol " << rtol_ << ", atol " << atol_);
}

GaussLaw::GaussLaw(interfaces::Simulation& simulation)
  : TableDiagnostic(CONFIG().out_dir + "/temporal/gauss_law.txt"), simulation(simulation)
{
  LOG("  GaussLaw table is added (the electrostatic step's own solve)");
}

PetscErrorCode GaussLaw::start()
{
  for (auto& sort : simulation.particles_) XCALL(sort->flush());
  if (solver_ >= 0) HIPCALL(xpic_set_poisson_solver(simulation.ctx, solver_)); // (no key: the context's default, CG)
  if (at_start_) {
    int its = 0;
    double o4[4];
    HIPCALL(xpic_gauss_clean(simulation.ctx, XPIC_E, rtol_, atol_, maxit_, nullptr, &its, o4));
    LOG("  Gauss law at start: |res| " << o4[0] << " -> " << o4[1] << ", " << its << " iterations, mean charge " << o4[2]);
  }
  if (simulation.scheme() != XPIC_ES) HIPCALL(xpic_set_gauss_clean(simulation.ctx, every_, rtol_, atol_, maxit_));
  return 0;
}

PetscErrorCode GaussLaw::add_columns(PetscInt t)
{
  double info[6], o4[4];
  HIPCALL(xpic_gauss_info(simulation.ctx, info));
  const bool cleaned = info[0] != cleans_seen_; // a clean ran since the last row: at the start, or inside this step
  cleans_seen_ = info[0];
  if (!cleaned) HIPCALL(xpic_gauss_residual(simulation.ctx, XPIC_E, nullptr, o4));
  add_int(6, "Time", t);
  add(13, "Res_before", "% .6e", cleaned ? info[2] : o4[1]);
  add(13, "Res_after", "% .6e", cleaned ? info[3] : o4[1]);
  add(13, "Mean_rho", "% .6e", cleaned ? info[4] : o4[2]);
  add_int(10, "Iterations", cleaned ? (long)info[5] : 0);
  return 0;
}

// ---- MomentumConservation (src/diagnostics/momentum_conservation.cpp): dP/dt against the force q E on the particles
MomentumConservation::MomentumConservation(interfaces::Simulation& simulation)
  : TableDiagnostic(CONFIG().out_dir + "/temporal/momentum_conservation.txt"), simulation(simulation)
{
}

PetscErrorCode MomentumConservation::calculate()
{
  const size_t n = simulation.particles_.size();
  std::vector<double> sums(6 * n);
  HIPCALL(xpic_momentum(simulation.ctx, sums.data()));
  P1.resize(n);
  QE.resize(n);
  P0.resize(n);
  for (size_t i = 0; i < n; ++i)
    for (int c = 0; c < 3; ++c) {
      P1[i][c] = sums[6 * i + c];
      QE[i][c] = sums[6 * i + 3 + c];
    }
  return 0;
}

PetscErrorCode MomentumConservation::initialize()
{
  XCALL(calculate());
  P0 = P1;
  return 0;
}

PetscErrorCode MomentumConservation::add_columns(PetscInt t)
{
  XCALL(calculate());
  add_int(6, "Time", t);
  auto length = [](const Vector3R& v) { return std::sqrt(v.squared()); };
  Vector3R total;
  for (size_t i = 0; i < P1.size(); ++i) {
    const std::string& name = simulation.particles_[i]->parameters.sort_name;
    static const char* axis[3] = {"x_", "y_", "z_"};
    for (int c = 0; c < 3; ++c) add(13, std::string("P") + axis[c] + name, "% .6e", P1[i][c]);
    for (int c = 0; c < 3; ++c) add(13, std::string("QE") + axis[c] + name, "% .6e", QE[i][c]);
    Vector3R defect, diff, mean;
    for (int c = 0; c < 3; ++c) {
      diff[c] = P1[i][c] - P0[i][c];
      mean[c] = P1[i][c] + P0[i][c];
      defect[c] = diff[c] / dt - QE[i][c]; // (p1 - p0) / dt - qe   :56
      total[c] += defect[c];
    }
    PetscReal freq = 0;
    if (const PetscReal denom = length(mean); std::abs(denom) > 1e-10 /* PETSC_SMALL */)
      freq = (length(diff) / denom) / (0.5 * dt);
    add(13, "N2dP_" + name, "% .6e", length(defect));
    add(13, "fP_" + name, "% .6e", freq);
    P0[i] = P1[i];
  }
  add(13, "N2dP", "% .6e", length(total));
  return 0;
}

// ---- Energy (src/diagnostics/energy.cpp:9-185; ecsimcorr::Energy src/impls/ecsimcorr/simulation.cpp:157-197)
Energy::Energy(interfaces::Simulation& simulation)
  : simulation(simulation), energy(CONFIG().out_dir + "/temporal/energy.txt"),
    energy_cons(CONFIG().out_dir + "/temporal/energy_conservation.txt")
{
  const size_t n = simulation.particles_.size();
  K.assign(n, 0);
  K0.assign(n, 0);
  std_K.assign(n, 0);
}

PetscErrorCode Energy::calculate()
{
  std::vector<double> out(4 + 2 * K.size());
  HIPCALL(xpic_energy(simulation.ctx, out.data()));
  E = out[0]; B = out[1]; std_E = out[2]; std_B = out[3];
  for (size_t i = 0; i < K.size(); ++i) { K[i] = out[4 + 2 * i]; std_K[i] = out[5 + 2 * i]; }
  return 0;
}

PetscErrorCode Energy::diagnose(PetscInt t)
{
  if (t == simulation.start) XCALL(calculate());
  E0 = E; B0 = B; K0 = K;
  XCALL(calculate());

  auto& particles = simulation.particles_;
  // fill_energy :111-135
  energy.add_int(6, "Time", t);
  energy.add(13, "wE", "% .6e", E);
  energy.add(13, "wB", "% .6e", B);
  for (size_t i = 0; i < K.size(); ++i) energy.add(13, "wK_" + particles[i]->parameters.sort_name, "% .6e", K[i]);
  energy.add(13, "sE", "% .6e", std_E);
  energy.add(13, "sB", "% .6e", std_B);
  for (size_t i = 0; i < K.size(); ++i) energy.add(13, "sK_" + particles[i]->parameters.sort_name, "% .6e", std_K[i]);

  // fill_energy_cons :137-185
  energy_cons.add_int(6, "Time", t);
  const PetscReal dE = E - E0, dB = B - B0;
  PetscReal dF = dE + dB, dK = 0;
  energy_cons.add(13, "dE", "% .6e", dE);
  energy_cons.add(13, "dB", "% .6e", dB);
  for (size_t i = 0; i < K.size(); ++i) {
    energy_cons.add(13, "dK_" + particles[i]->parameters.sort_name, "% .6e", K[i] - K0[i]);
    dK += K[i] - K0[i];
  }
  for (const auto& command : simulation.step_presets()) { // energy.cpp:156-178, in the step presets' order
    if (auto* damp = dynamic_cast<FieldsDamping*>(command.get())) {
      energy_cons.add(13, "Damped(E+B)", "% .6e", damp->get_damped_energy());
      dF += damp->get_damped_energy();
    }
    if (auto* injection = dynamic_cast<InjectParticles*>(command.get())) {
      const PetscReal wi = injection->get_ionized_energy(), we = injection->get_ejected_energy();
      energy_cons.add(13, "Inj_" + injection->get_ionized_name(), "% .6e", wi);
      energy_cons.add(13, "Inj_" + injection->get_ejected_name(), "% .6e", we);
      dK -= wi + we;
    }
    if (auto* remove = dynamic_cast<RemoveParticles*>(command.get())) {
      energy_cons.add(13, "Rm_" + remove->get_particles_name(), "% .6e", remove->get_removed_energy());
      dK += remove->get_removed_energy();
    }
  }
  energy_cons.add(13, "dE+dB+dK", "% .6e", dF + dK);
  if (simulation.scheme() == XPIC_ECSIMCORR) {
    PetscInt off = 3;
    PetscReal corr_w = 0.0;
    for (size_t i = 0; i < K.size(); ++i) {
      double s[6];
      HIPCALL(xpic_ecsimcorr_scalars(simulation.ctx, particles[i]->sort_id, s));
      const std::string& name = particles[i]->parameters.sort_name;
      energy_cons.add(13, "CWD_" + name, "% .6e", s[2], ++off);            // lambda_dK
      energy_cons.add(13, "PWD_" + name, "% .6e", s[3] - dt * s[0], ++off); // pred_dK - dt pred_w
      energy_cons.add(13, "LdK_" + name, "% .6e", s[4] - dt * s[1], ++off); // corr_dK - dt corr_w
      ++off;
      corr_w += s[1];
    }
    energy_cons.add(13, "WD", "% .6e", dK - dt * corr_w);
  }
  XCALL(energy.diagnose(t));
  XCALL(energy_cons.diagnose(t));
  return 0;
}
