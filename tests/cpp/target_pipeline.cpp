// target_pipeline.cpp — TraditionalRasterizer::draw over a framebuffer that stays on the device: several scenes in one pipeline, several
// meshes and shaders in one scene, the texture-slot map, structure changes between draws, the unbound-shader throw, partial clears.
// Every check compares the device vertex stage with the host one bit for bit (or with planes this program kept); the planes it dumps
// are compared with the oracle by tests/test_gpu_cpp_api.py, which builds the same frames through srz.scenes.Workload.
// Usage: target_pipeline <repository root> [<dump prefix>].  Exit codes: 0 ok, 3 = no GPU (the first constructor threw), 1 = wrong output.
#include <SoftRasterizer.hpp>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

namespace SR = SoftRasterizer;
using Pipe = std::shared_ptr<SR::TraditionalRasterizer>;

static const glm::vec3 Y(0.f, 1.f, 0.f), EYE(0.0f, 0.0f, 0.9f);
static const SR::Buffers BOTH = SR::Buffers::Color | SR::Buffers::Depth;
static const char *UNBOUND = "draw: a mesh with triangles has no shader bound (bindShader2Mesh)";

struct Placed { // a mesh and where the frames put it (srz.scenes.Workload: rotation about Y by 10 degrees a frame)
  std::string name;
  glm::vec3 t;
  float s;
};

struct Planes {
  std::vector<float> p[4];
  bool operator==(const Planes &o) const {
    for (int k = 0; k < 4; ++k)
      if (p[k].size() != o.p[k].size() || std::memcmp(p[k].data(), o.p[k].data(), p[k].size() * 4) != 0) return false;
    return true;
  }
};

static Planes planes_of(const Pipe &r) {
  Planes out;
  out.p[0] = r->zBuffer();
  for (int c = 0; c < 3; ++c) out.p[1 + c] = r->channel(c);
  return out;
}

static int fail(const char *what) {
  std::fprintf(stderr, "target_pipeline: WRONG: %s\n", what);
  return 1;
}

static bool add(const std::shared_ptr<SR::Scene> &sc, const std::string &path, const Placed &m, const char *shader) {
  if (!sc->addGraphicObj(path, m.name, Y, 0.0f, m.t, glm::vec3(m.s)) || !sc->startLoadingMesh(m.name)) return false;
  return shader == nullptr || sc->bindShader2Mesh(m.name, shader);
}

static void lights(const std::shared_ptr<SR::Scene> &sc) {
  sc->addLight("Light1", std::make_shared<SR::light_struct>(glm::vec3{0.9, 0.9, -0.9f}, glm::vec3{100, 100, 100}));
  sc->addLight("Light2", std::make_shared<SR::light_struct>(glm::vec3{0.f, 0.8f, 0.9f}, glm::vec3{50, 50, 50}));
}

static void pose(const std::shared_ptr<SR::Scene> &sc, const std::vector<Placed> &meshes, int frame) {
  for (const Placed &m : meshes) sc->setModelMatrix(m.name, Y, float((10 * frame) % 360), m.t, glm::vec3(m.s));
  sc->setViewMatrix(EYE, glm::vec3(0.0f), Y);
  sc->setProjectionMatrix(45.0f, 0.1f, 100.0f);
}

static bool dump(const char *prefix, const char *name, const Planes &pl) {
  if (!prefix) return true;
  std::FILE *fp = std::fopen((std::string(prefix) + name + ".f32").c_str(), "wb");
  if (!fp) return false;
  for (int k = 0; k < 4; ++k) std::fwrite(pl.p[k].data(), 4, pl.p[k].size(), fp);
  return std::fclose(fp) == 0;
}

static void print_stats(const char *name, const SR::TraditionalRasterizer::Stats &s) {
  std::printf("STATS %s n_tris=%llu n_culled=%llu pixel_tests=%llu fragments=%llu shaded=%llu visible=%llu visible_textured=%llu\n", name,
              (unsigned long long)s.n_tris, (unsigned long long)s.n_culled, (unsigned long long)s.pixel_tests, (unsigned long long)s.fragments,
              (unsigned long long)s.shaded, (unsigned long long)s.visible, (unsigned long long)s.visible_textured);
}

static bool same_stats(const SR::TraditionalRasterizer::Stats &a, const SR::TraditionalRasterizer::Stats &b) {
  return a.n_tris == b.n_tris && a.n_culled == b.n_culled && a.pixel_tests == b.pixel_tests && a.fragments == b.fragments &&
         a.shaded == b.shaded && a.visible == b.visible && a.visible_textured == b.visible_textured;
}

// frameBuffer8() after display() = the host rounding of the float planes (the rule of api_demo.cpp)
static bool resolved(const Pipe &r) {
  const auto &bgr = r->frameBuffer8();
  const size_t n = r->width() * r->height();
  for (size_t i = 0; i < n; ++i)
    for (int c = 0; c < 3; ++c) {
      long v = std::lrintf(r->channel(c)[i]);
      v = v < 0 ? 0 : (v > 255 ? 255 : v);
      if (bgr[i * 3 + c] != (unsigned char)v) return false;
    }
  return true;
}

// clear(Color|Depth) and draw() on the device-stage and on the host-stage pipeline: the planes are equal bit for bit -> *out
static bool both(const Pipe &dev, const Pipe &host, Planes *out) {
  for (const Pipe &r : {dev, host}) {
    r->clear(BOTH);
    r->draw(SR::Primitive::TRIANGLES);
  }
  *out = planes_of(dev);
  return *out == planes_of(host);
}

static bool throws_unbound(const Pipe &r) {
  try {
    r->draw(SR::Primitive::TRIANGLES);
  } catch (const std::runtime_error &e) {
    return std::string(e.what()) == UNBOUND;
  }
  return false;
}

static SR::Mesh *mesh_of(const std::shared_ptr<SR::Scene> &sc, const char *name) {
  auto obj = sc->getMeshObj(name);
  return obj ? dynamic_cast<SR::Mesh *>(obj->get()) : nullptr;
}

int main(int argc, char **argv) {
  const std::string assets = (argc > 1 ? std::string(argv[1]) : std::string(".")) + "/assets/models/";
  const char *prefix = argc > 2 ? argv[2] : nullptr;
  const std::string spot_obj = assets + "spot/spot_triangulated_good.obj", spot_png = assets + "spot/spot_texture.png";
  const std::string crate_obj = assets + "Crate/Crate1.obj", crate_png = assets + "Crate/Crate1.png", bunny_obj = assets + "bunny/bunny.obj";
  const int W = 101, H = 67; // odd: W * H is no multiple of 4
  Pipe dev, host;
  try {
    dev = std::make_shared<SR::TraditionalRasterizer>(W, H), host = std::make_shared<SR::TraditionalRasterizer>(W, H);
  } catch (const std::runtime_error &e) {
    std::fprintf(stderr, "runtime_error: %s\n", e.what());
    return 3;
  }
  try {
    host->device_vertex_stage = false;

    // ---- two scenes in one pipeline: spot TEXTURE + crate PHONG (two different textures), then the bunny NORMAL onto them
    const std::vector<Placed> one_meshes = {{"spot", glm::vec3(-0.15f, 0.0f, 0.0f), 0.3f}, {"Crate", glm::vec3(0.2f, -0.1f, 0.1f), 0.15f}};
    std::vector<Placed> two_meshes = {{"bunny", glm::vec3(-0.05f, -0.12f, 0.12f), 2.0f}};
    auto one = std::make_shared<SR::Scene>("one", EYE, glm::vec3(0.0f), Y), two = std::make_shared<SR::Scene>("two", EYE, glm::vec3(0.0f), Y);
    if (!one->addShader("spot_tex", spot_png, SR::SHADERS_TYPE::TEXTURE) || !one->addShader("crate_phong", crate_png, SR::SHADERS_TYPE::PHONG) ||
        !two->addShader("bunny_normal", spot_png, SR::SHADERS_TYPE::NORMAL))
      return fail("addShader");
    if (!add(one, spot_obj, one_meshes[0], "spot_tex") || !add(one, crate_obj, one_meshes[1], "crate_phong") ||
        !add(two, bunny_obj, two_meshes[0], "bunny_normal"))
      return fail("loading the meshes");
    lights(one), lights(two);
    for (const Pipe &r : {dev, host})
      if (!r->addScene(one) || !r->addScene(two) || r->addScene(two)) return fail("addScene");
    pose(one, one_meshes, 3), pose(two, two_meshes, 3);
    Planes first;
    if (!both(dev, host, &first)) return fail("two scenes: device vertex stage != host vertex stage");
    if (!dump(prefix, "two_scenes", first)) return fail("dump");
    dev->draw(SR::Primitive::TRIANGLES); // draw() never clears: both scenes again over their own picture change nothing
    if (!(planes_of(dev) == first)) return fail("two scenes drawn again over their own planes changed them");

    // ---- stats over incoming planes: the second scene's counting pass starts from the first scene's planes
    for (const Pipe &r : {dev, host}) {
      r->collect_stats = true;
      r->clear(BOTH);
      r->draw(SR::Primitive::TRIANGLES);
      r->collect_stats = false;
      if (!(planes_of(r) == first)) return fail("planes drawn with collect_stats differ from those drawn without");
    }
    print_stats("two_scenes", dev->last_stats);
    if (!same_stats(dev->last_stats, host->last_stats)) return fail("last_stats: device stage != host stage");
    dev->collect_stats = true; // ... and over a picture that is already there: nothing of the second pass may win a pixel twice
    dev->draw(SR::Primitive::TRIANGLES);
    dev->collect_stats = false;
    print_stats("two_scenes_again", dev->last_stats);
    if (!(planes_of(dev) == first)) return fail("a redraw with collect_stats changed the planes");

    // ---- display() at the odd size
    dev->clear(BOTH);
    dev->display(SR::Primitive::TRIANGLES);
    if (!(planes_of(dev) == first) || !resolved(dev)) return fail("display() at 101 x 67");

    // ---- texture slots: two shaders sharing one TextureLoader and a third with its own, at 128 x 96
    {
      Pipe tdev = std::make_shared<SR::TraditionalRasterizer>(128, 96), thost = std::make_shared<SR::TraditionalRasterizer>(128, 96);
      thost->device_vertex_stage = false;
      const std::vector<Placed> m = {{"spotA", glm::vec3(-0.2f, 0.05f, 0.0f), 0.25f}, {"Crate", glm::vec3(0.05f, -0.1f, 0.1f), 0.15f},
                                     {"spotB", glm::vec3(0.22f, 0.0f, 0.05f), 0.25f}};
      auto sc = std::make_shared<SR::Scene>("slots", EYE, glm::vec3(0.0f), Y);
      auto shared = std::make_shared<SR::TextureLoader>(spot_png);
      if (!sc->addShader("shared_a", shared, SR::SHADERS_TYPE::TEXTURE) || !sc->addShader("own", crate_png, SR::SHADERS_TYPE::TEXTURE) ||
          !sc->addShader("shared_b", shared, SR::SHADERS_TYPE::TEXTURE))
        return fail("addShader (slots)");
      if (!add(sc, spot_obj, m[0], "shared_a") || !add(sc, crate_obj, m[1], "own") || !add(sc, spot_obj, m[2], "shared_b"))
        return fail("loading the meshes (slots)");
      lights(sc);
      if (!tdev->addScene(sc) || !thost->addScene(sc)) return fail("addScene (slots)");
      pose(sc, m, 7);
      Planes pic;
      if (!both(tdev, thost, &pic)) return fail("texture slots: device vertex stage != host vertex stage");
      if (!dump(prefix, "texture_slots", pic)) return fail("dump");
      tdev->clear(BOTH);
      tdev->display(SR::Primitive::TRIANGLES);
      if (!(planes_of(tdev) == pic) || !resolved(tdev)) return fail("display() at 128 x 96");
    }

    // ---- structure changes between draws, each against the host-stage pipeline
    Planes got;
    const Placed extra{"Crate2", glm::vec3(-0.1f, 0.15f, 0.2f), 0.12f};
    if (!two->addShader("crate_normal", crate_png, SR::SHADERS_TYPE::NORMAL) || !add(two, crate_obj, extra, "crate_normal"))
      return fail("adding a mesh to a scene that was drawn");
    two_meshes.push_back(extra);
    pose(two, two_meshes, 3);
    if (!both(dev, host, &got)) return fail("a mesh added to a drawn scene: device != host");
    if (got == first) return fail("the added mesh does not show");
    const Planes with_extra = got;
    SR::Mesh *bunny = mesh_of(two, "bunny"), *crate2 = mesh_of(two, "Crate2");
    if (!bunny || !crate2) return fail("getMeshObj");
    const std::vector<glm::uvec3> bunny_faces = bunny->faces;
    bunny->faces.resize(bunny_faces.size() / 2);
    if (!both(dev, host, &got)) return fail("a face list shrunk in place: device != host");
    if (got == with_extra) return fail("the shrunk face list does not show");
    bunny->faces = bunny_faces;
    if (!both(dev, host, &got)) return fail("the face list restored: device != host");
    if (!(got == with_extra)) return fail("the face list restored: not the picture of before");
    crate2->faces.clear(); // a mesh without faces is skipped: the picture of before it was added
    if (!both(dev, host, &got)) return fail("a mesh emptied in place: device != host");
    if (!(got == first)) return fail("a mesh emptied in place: not the picture of before it was added");

    // ---- a mesh with faces and no shader bound: draw() throws in both modes, and the pipeline goes on afterwards
    const Placed unbound{"Crate3", glm::vec3(0.0f, 0.0f, 0.3f), 0.1f};
    if (!add(two, crate_obj, unbound, nullptr)) return fail("adding the unbound mesh");
    two_meshes.push_back(unbound);
    pose(two, two_meshes, 3);
    if (!throws_unbound(dev) || !throws_unbound(host)) return fail("a mesh with faces and no shader did not throw the documented error");
    SR::Mesh *crate3 = mesh_of(two, "Crate3");
    if (!crate3) return fail("getMeshObj");
    crate3->faces.clear();
    pose(one, one_meshes, 5), pose(two, two_meshes, 5);
    if (!both(dev, host, &got)) return fail("after the throw: device != host");
    if (!dump(prefix, "after_throw", got)) return fail("dump");

    // ---- clear(Color) alone keeps z and zeroes the colours
    dev->clear(SR::Buffers::Color);
    const Planes cleared = planes_of(dev);
    if (std::memcmp(cleared.p[0].data(), got.p[0].data(), got.p[0].size() * 4) != 0) return fail("clear(Color) changed z");
    for (int c = 1; c < 4; ++c)
      for (float v : cleared.p[c]) {
        uint32_t w;
        std::memcpy(&w, &v, 4);
        if (w != 0) return fail("clear(Color) left a colour word that is not +0.0");
      }
    size_t covered = 0;
    for (float z : cleared.p[0]) covered += std::isfinite(z) ? 1 : 0;
    std::printf("covered=%zu\n", covered);
    return covered ? 0 : fail("nothing covered");
  } catch (const std::runtime_error &e) { // (the pipelines exist: whatever throws from here on is a wrong result, not a missing GPU)
    std::fprintf(stderr, "runtime_error: %s\n", e.what());
    return 1;
  }
}
