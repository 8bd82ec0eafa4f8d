// amwg_rtc.hip -- runtime compilation of a translated closure: the program handed to hiprtc (user_program), the on-disk cache of code objects,
// what the generated source says about itself (source_traits), and the compile-and-load of the kernel of a sampler's plan (load_user_kernel).
#include <hip/hiprtc.h>
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>

#include "amwg_host.h"

// The kernel headers as text (amwg_rtc_headers.c, .incbin): hiprtc compiles a translated closure
// together with the very same step kernel source the built-in models are compiled from.
extern "C" {
extern const char amwg_hdr_stdint[], amwg_hdr_types[], amwg_hdr_math[], amwg_hdr_div[], amwg_hdr_ld[], amwg_hdr_philox[],
    amwg_hdr_kernel[], amwg_hdr_user[], amwg_hdr_twoval[], amwg_hdr_kval[], amwg_hdr_trig[], amwg_hdr_pass[], amwg_hdr_rows[], amwg_hdr_window[], amwg_hdr_gtail[],
    amwg_hdr_user_kernels[], amwg_hdr_user_dataset[], amwg_hdr_select[], amwg_hdr_pointwise[], amwg_hdr_pointwise_types[];
}

// ---- hiprtc: a translated closure + its step kernels (amwg_user_kernels.h) -> code object for one (lanes, workgroup) geometry
static std::string user_program(const char *source, int lanes, int block) {
  return "#include \"amwg_kernel.h\"\n#include \"amwg_user.h\"\n#define AMWG_USER_LANES " + std::to_string(lanes) + "\n#define AMWG_USER_BLOCK " + std::to_string(block) + "\n" +
         source + "\n#include \"amwg_user_kernels.h\"\n";
}

// ---- on-disk cache of compiled code objects.  hiprtc takes ~0.6 s per closure and geometry; the reference's own use -- one chain, a
// script run once (README.md:41-42) -- would pay that at every start.  Key = everything that determines the code object: the program
// text, the embedded kernel headers, the compile options, the target, the hiprtc version.  Files: <dir>/<128-bit key hash>.hsaco, each
// carrying the key's length and a second hash, written to a temporary name and renamed (concurrent processes never see a partial file).
// Directory: $AMWG_CACHE_DIR, else $XDG_CACHE_HOME/amwg, else $HOME/.cache/amwg; AMWG_CACHE_DIR="" (empty) or an unwritable directory
// disables it silently -- the cache is an optimisation, never a requirement.
namespace {
struct CacheKey { uint64_t h1, h2, h3; uint64_t len; };
CacheKey hash_key(const std::vector<std::string> &parts) {
  CacheKey k{0xcbf29ce484222325ull, 0x84222325cbf29ce4ull, 0x9e3779b97f4a7c15ull, 0};
  for (const std::string &p : parts) {
    for (unsigned char c : p) {
      k.h1 = (k.h1 ^ c) * 0x100000001b3ull;                                   // FNV-1a
      k.h2 = (k.h2 + c + (k.h2 << 6) + (k.h2 >> 2)) * 0xff51afd7ed558ccdull;  // an unrelated mix
      k.h3 = ((k.h3 << 5) | (k.h3 >> 59)) ^ (c * 0xc4ceb9fe1a85ec53ull);
    }
    k.h1 = (k.h1 ^ 0xff) * 0x100000001b3ull;                                  // part separator
    k.len += p.size() + 1;
  }
  return k;
}
std::string cache_dir() {
  if (const char *d = getenv("AMWG_CACHE_DIR")) return d;       // (empty string: disabled)
  if (const char *x = getenv("XDG_CACHE_HOME")) if (*x) return std::string(x) + "/amwg";
  if (const char *h = getenv("HOME")) if (*h) return std::string(h) + "/.cache/amwg";
  return "";
}
void make_dirs(const std::string &path) {      // mkdir -p; the cache directory itself is private to the user (code objects are loaded from it)
  for (size_t i = 1; i <= path.size(); ++i)
    if (i == path.size() || path[i] == '/') (void)mkdir(path.substr(0, i).c_str(), i == path.size() ? 0700 : 0755);
}
// Code objects are LOADED from this directory: it is used only while it belongs to this user and nobody else can write to it.  An existing
// directory with group / other write bits is tightened to 0700 when it is ours (a leftover 0755 from before round 4 included); one that
// belongs to somebody else, or is not a directory (a symlink is not followed), switches the cache off.  The payload sum in a file's header
// guards against damage, not against a planted file -- this check, O_NOFOLLOW and the owner test in cache_read are what guard against that.
bool cache_dir_trusted(const std::string &dir) {
  struct stat st;
  if (lstat(dir.c_str(), &st) != 0 || !S_ISDIR(st.st_mode) || st.st_uid != geteuid()) return false;
  if ((st.st_mode & (S_IWGRP | S_IWOTH)) != 0 && chmod(dir.c_str(), 0700) != 0) return false;
  return true;
}
uint64_t payload_sum(const std::vector<char> &code) {      // FNV-1a over the code bytes: a damaged file is recompiled, not handed to the loader
  uint64_t h = 0xcbf29ce484222325ull;
  for (unsigned char c : code) h = (h ^ c) * 0x100000001b3ull;
  return h;
}
const char kCacheMagic[8] = {'A', 'M', 'W', 'G', 'c', 'o', '0', '2'};
bool cache_read(const std::string &file, const CacheKey &k, std::vector<char> *code) {
  const int fd = open(file.c_str(), O_RDONLY | O_NOFOLLOW | O_CLOEXEC);
  if (fd < 0) return false;
  struct stat st;
  if (fstat(fd, &st) != 0 || !S_ISREG(st.st_mode) || st.st_uid != geteuid() || (st.st_mode & (S_IWGRP | S_IWOTH)) != 0) { close(fd); return false; }      // not ours: not loaded (and not removed)
  FILE *f = fdopen(fd, "rb");
  if (!f) { close(fd); return false; }
  char magic[8];
  uint64_t hdr[4] = {0, 0, 0, 0}, n = 0;
  bool ok = fread(magic, 1, 8, f) == 8 && memcmp(magic, kCacheMagic, 8) == 0 && fread(hdr, 8, 4, f) == 4 && fread(&n, 8, 1, f) == 1 &&
            hdr[0] == k.h2 && hdr[1] == k.h3 && hdr[2] == k.len && n > 0 && n < (1ull << 31);
  if (ok) { code->resize((size_t)n); ok = fread(code->data(), 1, (size_t)n, f) == (size_t)n && payload_sum(*code) == hdr[3]; }
  fclose(f);
  if (!ok) (void)remove(file.c_str());      // stale format, truncated or damaged: gone, the caller compiles
  return ok;
}
void cache_write(const std::string &dir, const std::string &file, const CacheKey &k, const std::vector<char> &code) {
  make_dirs(dir);
  if (!cache_dir_trusted(dir)) return;
  const std::string tmp = file + ".tmp." + std::to_string((long)getpid());
  const int fd = open(tmp.c_str(), O_WRONLY | O_CREAT | O_EXCL | O_NOFOLLOW | O_CLOEXEC, 0600);
  if (fd < 0) return;
  FILE *f = fdopen(fd, "wb");
  if (!f) { close(fd); (void)remove(tmp.c_str()); return; }
  const uint64_t hdr[4] = {k.h2, k.h3, k.len, payload_sum(code)}, n = code.size();
  const bool ok = fwrite(kCacheMagic, 1, 8, f) == 8 && fwrite(hdr, 8, 4, f) == 4 && fwrite(&n, 8, 1, f) == 1 && fwrite(code.data(), 1, code.size(), f) == code.size();
  if (fclose(f) != 0 || !ok || rename(tmp.c_str(), file.c_str()) != 0) (void)remove(tmp.c_str());
}
std::atomic<int> g_cache_hits{0}, g_cache_misses{0};      // (samplers may be created from several threads)
}  // namespace

static void dump_code_object(const std::vector<char> &code) {      // development aid: inspect the ISA with llvm-objdump
  if (const char *dump = getenv("AMWG_DUMP_CODE_OBJECT")) {
    if (FILE *f = fopen(dump, "wb")) { fwrite(code.data(), 1, code.size(), f); fclose(f); }
  }
}

// use_cache = false: compile even if the on-disk cache has the object (the caller found the cached one unloadable)
// datasets: with the dataset twins (amwg_user_dataset.h) compiled in -- one more compile option, hence one more part of the cache key
// pointwise = true: prog_src is a closure's pointwise program (pointwise_program) -- the same options and cache, three more headers (amwg_select.h, amwg_pointwise.h, amwg_pointwise_types.h)
static int compile_program(const std::string &prog_src, const char *arch, std::vector<char> *code, bool datasets, bool use_cache, bool pointwise) {
  static const char *names[] = {"amwg_stdint.h", "amwg_types.h", "amwg_math.h", "amwg_div.h", "amwg_ld.h", "amwg_philox.h", "amwg_kernel.h", "amwg_user.h",
                                "amwg_twoval.h", "amwg_kval.h", "amwg_trig.h", "amwg_pass.h", "amwg_rows.h", "amwg_window.h", "amwg_gtail.h", "amwg_user_kernels.h", "amwg_user_dataset.h",
                                "amwg_select.h", "amwg_pointwise.h", "amwg_pointwise_types.h"};
  const char *texts[] = {amwg_hdr_stdint, amwg_hdr_types, amwg_hdr_math, amwg_hdr_div, amwg_hdr_ld, amwg_hdr_philox, amwg_hdr_kernel, amwg_hdr_user,
                         amwg_hdr_twoval, amwg_hdr_kval, amwg_hdr_trig, amwg_hdr_pass, amwg_hdr_rows, amwg_hdr_window, amwg_hdr_gtail, amwg_hdr_user_kernels, amwg_hdr_user_dataset,
                         amwg_hdr_select, amwg_hdr_pointwise, amwg_hdr_pointwise_types};
  const int kHeaders = (int)(sizeof(texts) / sizeof(texts[0])) - (pointwise ? 0 : 3);      // (a step-kernel program sees, and is keyed by, the headers it always had)
#if defined(AMWG_AUDIT)      // (libamwg_audit.so: the certified kernels of translated closures record |A - E| / eps as the built-in families' do)
  const char *const kOpts[] = {"-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wno-unused-value", "-DAMWG_AUDIT=1"};
#elif defined(AMWG_X_PHASES)      // (the phase-clock development build: translated closures are clocked too)
  const char *const kOpts[] = {"-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wno-unused-value", "-DAMWG_X_PHASES=1"};
#else
  const char *const kOpts[] = {"-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wno-unused-value", "-falign-loops=64"};
#endif
  static const char *const kDatasetsOpt = "-DAMWG_USER_DATASETS=1";
  // the on-disk cache (see above)
  std::string dir = cache_dir(), file;
  CacheKey key{};
  if (!dir.empty()) {
    int rt_major = 0, rt_minor = 0;
    (void)hiprtcVersion(&rt_major, &rt_minor);
    std::vector<std::string> parts = {prog_src, arch, "hiprtc " + std::to_string(rt_major) + "." + std::to_string(rt_minor)};
    for (const char *o : kOpts) parts.push_back(o);
    if (datasets) parts.push_back(kDatasetsOpt);
    for (int h = 0; h < kHeaders; ++h) parts.push_back(texts[h]);
    key = hash_key(parts);
    char name[64];
    snprintf(name, sizeof name, "/%016llx%016llx.hsaco", (unsigned long long)key.h1, (unsigned long long)key.h2);
    file = dir + name;
    if (use_cache && cache_dir_trusted(dir) && cache_read(file, key, code)) { ++g_cache_hits; dump_code_object(*code); return AMWG_OK; }
    if (!use_cache) (void)remove(file.c_str());
  }
  ++g_cache_misses;
  hiprtcProgram prog = nullptr;
  hiprtcResult r = hiprtcCreateProgram(&prog, prog_src.c_str(), "amwg_user_model.hip", kHeaders, texts, names);
  if (r != HIPRTC_SUCCESS) return amwg_fail(AMWG_EHIP, "hiprtcCreateProgram failed: %s", hiprtcGetErrorString(r));
  const std::string arch_opt = std::string("--offload-arch=") + arch;
  // same floating-point contract as the Makefile: one rounding per operation, no fused contraction
  std::vector<const char *> opts = {arch_opt.c_str()};
  for (const char *o : kOpts) opts.push_back(o);
  if (datasets) opts.push_back(kDatasetsOpt);
  r = hiprtcCompileProgram(prog, (int)opts.size(), opts.data());
  if (r != HIPRTC_SUCCESS) {
    size_t n = 0;
    hiprtcGetProgramLogSize(prog, &n);
    std::string log(n ? n : 1, '\0');
    if (n) hiprtcGetProgramLog(prog, &log[0]);
    hiprtcDestroyProgram(&prog);
    g_err = std::string(pointwise ? "the pointwise terms of the translated log_post did not compile (hiprtc): " : "the translated log_post did not compile (hiprtc): ") + log;
    return AMWG_EINVAL;
  }
  size_t cs = 0;
  hiprtcGetCodeSize(prog, &cs);
  code->resize(cs);
  hiprtcGetCode(prog, code->data());
  hiprtcDestroyProgram(&prog);
  if (!file.empty()) cache_write(dir, file, key, *code);
  dump_code_object(*code);
  return AMWG_OK;
}

static int compile_user(const char *source, int lanes, int block, const char *arch, std::vector<char> *code, bool datasets, bool use_cache = true) {
  return compile_program(user_program(source, lanes, block), arch, code, datasets, use_cache, false);
}

// ---- hiprtc: a translated closure + its pointwise terms (translate.js pointwisePlan: struct UserTerms) + the kernels of amwg_pointwise.h -> one code object
static std::string pointwise_program(const char *source, const char *terms) {
  return std::string("#include \"amwg_kernel.h\"\n#include \"amwg_user.h\"\n") + source + "\n" + terms + "\n#define AMWG_POINTWISE_USER 1\n#include \"amwg_pointwise.h\"\n";
}
static int compile_pointwise(const char *source, const char *terms, const char *arch, std::vector<char> *code, bool use_cache = true) {
  return compile_program(pointwise_program(source, terms), arch, code, false, use_cache, true);
}

// What the generated source of a translated closure (translate.js) states about itself, read off its markers: the row plan (kRowN, kRowGroups, kRowSweep,
// kRowCert; -1 = no such marker), the certified tail (kCertifiedTail, kTailN), the certified Poisson tail (kPoisTail, kTailN) and the certified logistic tail (kLogitTail, kTailN); 0 = none;
// and whether those two tails read their data-dependent constants from an array of the dataset (kTailPerDataset: translate.js tail_consts_array) rather than from the text.
SourceTraits source_traits(const char *src) {
  auto int_after = [&](const char *key) -> long {
    const char *q = strstr(src, key);
    return q ? strtol(q + strlen(key), nullptr, 10) : -1;
  };
  auto tail_n = [&](const char *marker) { const long n = strstr(src, marker) ? int_after("kTailN = ") : 0; return n > 0 && n < (1l << 28) ? (int)n : 0; };
  return SourceTraits{int_after("kRowN = "), int_after("kRowGroups = "), strstr(src, "kRowSweep = true") != nullptr, strstr(src, "kRowCert = true") != nullptr,
                      tail_n("kCertifiedTail = true"), tail_n("kPoisTail = true"), tail_n("kLogitTail = true"), strstr(src, "kTailPerDataset = true") != nullptr};
}

// ---- compile for the adopted plan (cached per process by source text + geometry + arch) and load on the sampler's device
int load_user_kernel(amwg_sampler *s, const char *source, const char *arch) {
  static std::mutex mu;
  static std::map<std::string, std::vector<char>> cache;
  const LaunchPlan &p = s->plan;
  const bool datasets = s->n_datasets > 1;      // (a dataset sampler: the code object with the twins, and the twin of the plan's kernel)
  const std::string key = std::string(arch) + "|" + std::to_string(p.lanes) + "|" + std::to_string(p.block) + (datasets ? "|ds|" : "|") + source;
  const std::string fn_name = std::string(info(p.variant).name) + (datasets ? "_ds" : "");
  std::lock_guard<std::mutex> lock(mu);
  auto it = cache.find(key);
  if (it == cache.end()) {
    std::vector<char> code;
    TRYB(compile_user(source, p.lanes, p.block, arch, &code, datasets));
    it = cache.emplace(key, std::move(code)).first;
  }
  if (s->user_module) return AMWG_OK;      // (autotune hands back the module it kept)
  auto load = [&]() {
    const hipError_t e = hipModuleLoadData(&s->user_module, it->second.data());
    return e == hipSuccess ? hipModuleGetFunction(&s->user_fn, s->user_module, fn_name.c_str()) : e;
  };
  hipError_t e = load();
  if (e != hipSuccess) {
    // the cache is never a requirement: an object the loader refuses (a planted or half-written file that still passed the checks, another
    // driver) is dropped and the closure compiled afresh, once
    (void)hipGetLastError();
    if (s->user_module) { (void)hipModuleUnload(s->user_module); s->user_module = nullptr; }
    TRYB(compile_user(source, p.lanes, p.block, arch, &it->second, datasets, false));
    e = load();
    if (e != hipSuccess) return amwg_fail(AMWG_EHIP, "loading the compiled log_post failed: %s", hipGetErrorString(e));
  }
  // workgroups of this kernel use up to the whole 160 KB LDS of a CU; not every runtime needs (or accepts) the opt-in for module functions
  (void)hipFuncSetAttribute(reinterpret_cast<const void *>(s->user_fn), hipFuncAttributeMaxDynamicSharedMemorySize, p.lds);
  (void)hipGetLastError();
  return AMWG_OK;
}

// ---- the pointwise code object of a sampler (amwg_set_pointwise): compiled at the first WAIC / LOO call, loaded on the sampler's device, kept until destroy
int load_pointwise(amwg_sampler *s, const char *arch) {
  static std::mutex mu;
  std::lock_guard<std::mutex> lock(mu);      // (taken first: two calls on one sampler must not both find no module)
  if (s->pw_module) return AMWG_OK;
  std::vector<char> code;
  TRYB(compile_pointwise(s->user_source.c_str(), s->pw_terms.c_str(), arch, &code));
  static const char *const kEntries[4] = {"amwg_pw_waic_partial", "amwg_pw_waic_loglik", "amwg_pw_loo_hist", "amwg_pw_loo_compact"};
  auto load = [&]() {
    hipError_t e = hipModuleLoadData(&s->pw_module, code.data());
    for (int k = 0; k < 4 && e == hipSuccess; ++k) e = hipModuleGetFunction(&s->pw_fn[k], s->pw_module, kEntries[k]);
    return e;
  };
  hipError_t e = load();
  if (e != hipSuccess) {      // (as load_user_kernel: an object the loader refuses is compiled afresh, once)
    (void)hipGetLastError();
    if (s->pw_module) { (void)hipModuleUnload(s->pw_module); s->pw_module = nullptr; }
    TRYB(compile_pointwise(s->user_source.c_str(), s->pw_terms.c_str(), arch, &code, false));
    e = load();
    if (e != hipSuccess) {
      if (s->pw_module) { (void)hipModuleUnload(s->pw_module); s->pw_module = nullptr; }
      return amwg_fail(AMWG_EHIP, "loading the compiled pointwise terms failed: %s", hipGetErrorString(e));
    }
  }
  return AMWG_OK;
}

extern "C" {

int amwg_compile_pointwise(const char *source, const char *terms_source, const char *arch, size_t *code_bytes) {
  if (!source || !terms_source || !arch) return amwg_fail(AMWG_EINVAL, "amwg_compile_pointwise: null argument");
  std::vector<char> code;
  int rc = compile_pointwise(source, terms_source, arch, &code);
  if (rc == AMWG_OK && code_bytes) *code_bytes = code.size();
  return rc;
}

int amwg_code_cache_stats(int64_t *hits, int64_t *misses, char *dir, size_t dir_capacity) {
  if (hits) *hits = g_cache_hits;
  if (misses) *misses = g_cache_misses;
  if (dir && dir_capacity) snprintf(dir, dir_capacity, "%s", cache_dir().c_str());
  return AMWG_OK;
}

int amwg_compile_user(const char *source, int32_t lanes_per_chain, int32_t block_threads, const char *arch, size_t *code_bytes) {
  if (!source || !arch) return amwg_fail(AMWG_EINVAL, "amwg_compile_user: null argument");
  std::vector<char> code;
  int rc = compile_user(source, lanes_per_chain, block_threads, arch, &code, false);
  if (rc == AMWG_OK && code_bytes) *code_bytes = code.size();
  return rc;
}

int amwg_compile_user_datasets(const char *source, int32_t lanes_per_chain, int32_t block_threads, const char *arch, size_t *code_bytes) {
  if (!source || !arch) return amwg_fail(AMWG_EINVAL, "amwg_compile_user_datasets: null argument");
  std::vector<char> code;
  int rc = compile_user(source, lanes_per_chain, block_threads, arch, &code, true);
  if (rc == AMWG_OK && code_bytes) *code_bytes = code.size();
  return rc;
}

}  // extern "C"
