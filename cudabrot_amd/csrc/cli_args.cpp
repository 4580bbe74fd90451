// cli_args.cpp -- the parser of the `cudabrot` command line (cli_args.h): the reference's flags and messages
// (cudabrot.cu:579-754: usage :579-620, flags :662-754; usage -> exit 0) and the extension flags, which the reference
// answers with its usage text.  Everything a flag is lies in two tables: the flag table (name, kind of value, store;
// a store returns the message of a bad value) and, for the flags that select a render of their own, the refusal table
// (which other flags that render does not combine with, and in which order that is said).
#include "cli_args.h"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <functional>
#include <vector>

namespace cb {
namespace {

// One of zr, zi, cr, ci at `text`, followed by `after` -> its column of P (else -1); *rest: behind `after`.
int axis_of(const char *text, char after, const char **rest) {
  static const char *const kNames[4] = {"zr", "zi", "cr", "ci"};
  for (int j = 0; j < 4; ++j) {
    if (strncmp(text, kNames[j], 2) == 0 && text[2] == after) {
      *rest = text + (after ? 3 : 2);
      return j;
    }
  }
  return -1;
}

// --project a,b,c,d:e,f,g,h: eight finite numbers, strtod's syntax (hexfloats included).
bool parse_projection(const char *text, double out[8]) {
  const char *at = text;
  for (int j = 0; j < 8; ++j) {
    if (*at == 0 || *at == ' ' || *at == '\t') return false;  // (strtod would skip blanks)
    char *end = nullptr;
    out[j] = strtod(at, &end);
    if (end == at || !isfinite(out[j]) || *end != (j == 7 ? 0 : (j == 3 ? ':' : ','))) return false;
    at = end + 1;
  }
  return true;
}

// --julia RE,IM: two finite numbers in [-2, 2], strtod's syntax (hexfloats included).
bool parse_julia(const char *text, double out[2]) {
  const char *at = text;
  for (int j = 0; j < 2; ++j) {
    if (*at == 0 || *at == ' ' || *at == '\t') return false;  // (strtod would skip blanks)
    char *end = nullptr;
    out[j] = strtod(at, &end);
    if (end == at || !(out[j] >= -2.0 && out[j] <= 2.0) || *end != (j == 1 ? 0 : ',')) return false;
    at = end + 1;
  }
  return true;
}

// --depth ROW:MIN:MAX[:N]: ROW an axis name or four finite numbers a,b,c,d, MIN < MAX finite, N decimal digits, 1 ..
// CB_DEPTH_MAX_SLICES (1 where it is left out); the numbers in strtod's syntax (hexfloats included).
bool parse_depth(const char *text, cb_depth *out) {
  const char *at = text;
  const int axis = axis_of(at, ':', &at);
  for (int j = 0; j < 4; ++j) {
    if (axis >= 0) {
      out->row[j] = j == axis ? 1.0 : 0.0;
      continue;
    }
    if (*at == 0 || *at == ' ' || *at == '\t') return false;  // (strtod would skip blanks)
    char *end = nullptr;
    out->row[j] = strtod(at, &end);
    if (end == at || !isfinite(out->row[j]) || *end != (j == 3 ? ':' : ',')) return false;
    at = end + 1;
  }
  double bounds[2];
  for (int j = 0; j < 2; ++j) {
    if (*at == 0 || *at == ' ' || *at == '\t') return false;
    char *end = nullptr;
    bounds[j] = strtod(at, &end);
    if (end == at || !isfinite(bounds[j]) || (j == 0 ? *end != ':' : (*end != ':' && *end != 0))) return false;
    at = *end ? end + 1 : end;
    if (j == 1 && *end == ':' && *at == 0) return false;  // a colon and no N
  }
  if (!(bounds[0] < bounds[1])) return false;
  long n = 1;
  if (*at != 0) {
    n = 0;
    for (; *at >= '0' && *at <= '9'; ++at) {
      n = n * 10 + (*at - '0');
      if (n > CB_DEPTH_MAX_SLICES) return false;
    }
    if (*at != 0 || n < 1) return false;
  }
  out->min = bounds[0];
  out->max = bounds[1];
  out->slices = (int) n;
  return true;
}

// --palette K:RRGGBB[,K:RRGGBB...]: 1 to CB_PALETTE_MAX_STOPS stops, K decimal digits and strictly ascending, the colour
// six hex digits.  Returns the number of stops, 0 for anything else.
int parse_palette(const char *text, cb_palette_stop out[CB_PALETTE_MAX_STOPS]) {
  const char *at = text;
  int n = 0;
  for (;;) {
    if (n == CB_PALETTE_MAX_STOPS || *at < '0' || *at > '9') return 0;
    long k = 0;
    for (; *at >= '0' && *at <= '9'; ++at) {
      k = k * 10 + (*at - '0');
      if (k > 0x7fffffffL) return 0;
    }
    if (*at++ != ':' || (n > 0 && k <= out[n - 1].k)) return 0;
    int v[3] = {0, 0, 0};
    for (int j = 0; j < 6; ++j, ++at) {
      const char ch = *at;
      const int digit = (ch >= '0' && ch <= '9') ? ch - '0' : (ch >= 'a' && ch <= 'f') ? ch - 'a' + 10 : (ch >= 'A' && ch <= 'F') ? ch - 'A' + 10 : -1;
      if (digit < 0) return 0;
      v[j / 2] = v[j / 2] * 16 + digit;
    }
    out[n++] = {(int) k, v[0], v[1], v[2]};
    if (*at == 0) return n;
    if (*at++ != ',') return 0;
  }
}

// --rotate X,Y:DEG on the current matrix: both rows are rotated in the (X, Y) coordinate plane, by cb_rotate_projection
// (host_abi.cpp; an integer multiple of 90 degrees is exact).
bool rotate_projection(const char *text, double p[8]) {
  const char *rest = nullptr;
  const int x = axis_of(text, ',', &rest);
  const int y = x < 0 ? -1 : axis_of(rest, ':', &rest);
  if (x < 0 || y < 0 || x == y || *rest == 0 || *rest == ' ' || *rest == '\t') return false;
  char *end = nullptr;
  const double degrees = strtod(rest, &end);
  if (end == rest || *end != 0 || !isfinite(degrees)) return false;
  return cb_rotate_projection(p, x, y, degrees) == 0;
}

// --sweep X,Y:DEG0:DEG1:F: two different axes, two finite angles in strtod's syntax (hexfloats included), F decimal
// digits, 1 .. CB_FRAMES_MAX.
bool parse_sweep(const char *text, Sweep *out) {
  const char *at = nullptr;
  const int x = axis_of(text, ',', &at);
  const int y = x < 0 ? -1 : axis_of(at, ':', &at);
  if (x < 0 || y < 0 || x == y) return false;
  double degrees[2];
  for (int j = 0; j < 2; ++j) {
    if (*at == 0 || *at == ' ' || *at == '\t') return false;  // (strtod would skip blanks)
    char *end = nullptr;
    degrees[j] = strtod(at, &end);
    if (end == at || !isfinite(degrees[j]) || *end != ':') return false;
    at = end + 1;
  }
  long n = 0;
  if (*at == 0) return false;
  for (; *at >= '0' && *at <= '9'; ++at) {
    n = n * 10 + (*at - '0');
    if (n > CB_FRAMES_MAX) return false;
  }
  if (*at != 0 || n < 1) return false;
  *out = {x, y, degrees[0], degrees[1], (int) n};
  return true;
}

// --density-filter R[:ALPHA[:N0]]: R and N0 decimal digits, ALPHA a number in strtod's syntax; the ranges are
// cb_density_thresholds', which also refuses a table that starts at 2^22 or above.
bool parse_density(const char *text, DensityFilter *out) {
  const char *at = text;
  DensityFilter d;
  long r = 0;
  if (*at < '0' || *at > '9') return false;
  for (; *at >= '0' && *at <= '9'; ++at) {
    r = r * 10 + (*at - '0');
    if (r > CB_DENSITY_MAX_RADIUS) return false;
  }
  d.radius = (int) r;
  if (*at == ':') {
    ++at;
    if (*at == 0 || *at == ' ' || *at == '\t') return false;  // (strtod would skip blanks)
    char *end = nullptr;
    d.alpha = strtod(at, &end);
    if (end == at || (*end != 0 && *end != ':')) return false;
    at = end;
    if (*at == ':') {
      ++at;
      unsigned long long n0 = 0;
      if (*at < '0' || *at > '9') return false;
      for (; *at >= '0' && *at <= '9'; ++at) {
        n0 = n0 * 10 + (unsigned long long) (*at - '0');
        if (n0 > (1ull << 20)) return false;
      }
      d.n0 = n0;
    }
  }
  uint64_t table[CB_DENSITY_MAX_RADIUS + 1];
  if (*at != 0 || d.radius < 1 || cb_density_thresholds(d.radius, d.alpha, d.n0, table) != 0) return false;
  *out = d;
  return true;
}

// --local-equalize TX[xTY][:CLIP]: TX and TY digits from 1 to 16, TY = TX where left out; CLIP 0 or from 1 to 256,
// rounded to 1/256, 4 where left out.
bool parse_local_equalize(const char *text, LocalEqualize *out) {
  const char *at = text;
  long side[2] = {0, 0};
  for (int k = 0; k < 2; ++k) {
    if (*at < '0' || *at > '9') return false;
    for (; *at >= '0' && *at <= '9'; ++at) {
      side[k] = side[k] * 10 + (*at - '0');
      if (side[k] > CB_LOCAL_EQUALIZE_MAX_TILES) return false;
    }
    if (side[k] < 1) return false;
    if (k == 0 && *at != 'x') {
      side[1] = side[0];
      break;
    }
    if (k == 0) ++at;
  }
  double clip = 4.0;
  if (*at == ':') {
    ++at;
    if (*at == 0 || *at == ' ' || *at == '\t') return false;  // (strtod would skip blanks)
    char *end = nullptr;
    clip = strtod(at, &end);
    if (end == at) return false;
    at = end;
  }
  if (*at != 0 || !(clip == 0.0 || (clip >= 1.0 && clip <= 256.0))) return false;
  out->tx = (int) side[0];
  out->ty = (int) side[1];
  out->clip_q = (uint32_t) floor(clip * 256.0 + 0.5);
  return true;
}

// The usage text is the command's documented interface (cudabrot.cu:579-620) and is printed as is.
const char kUsageBody[] =
    "Options may be one or more of the following:\n"
    "  --help: Prints these instructions.\n"
    "  -d <device number>: Sets which GPU to use. Defaults to GPU 0.\n"
    "  -o <output file name>: If provided, the rendered image will be saved\n"
    "     to a .pgm file with the given name. Otherwise, saves the image\n"
    "     to output.pgm.\n"
    "  -m <max escape iterations>: The maximum number of iterations to use\n"
    "     before giving up on seeing whether a point escapes.\n"
    "  -c <min escape iterations>: If a point escapes before this number of\n"
    "     iterations, it will be ignored.\n"
    "  -g <gamma correction>: A gamma-correction value to use on the\n"
    "     resulting image. If negative, no gamma correction will occur.\n"
    "  -t <seconds to run>: A number of seconds to run the calculation for.\n"
    "     Defaults to 10.0. If negative, the program will run continuously\n"
    "     and will terminate (saving the image) when it receives a SIGINT.\n"
    "  -w <width>: The width of the output image, in pixels. Defaults to\n"
    "     1000.\n"
    "  -h <height>: The height of the output image, in pixels. Defaults to\n"
    "     1000.\n"
    "  -s <save/load file>: If provided, this gives a file name into which\n"
    "     the rendering buffer will be saved, for future continuation.\n"
    "     If the program is loaded and the file exists, the buffer will be\n"
    "     filled with the contents of the file, but the dimensions must\n"
    "     match. Note that this file may be huge for high-resolution images.\n"
    "  --white-clip <percent>: Scales the image against the count that this\n"
    "     percentage of the nonzero pixels may exceed, rather than against\n"
    "     the largest count; brighter pixels saturate. From 0 (the default,\n"
    "     off) to below 100.\n"
    "  --density-filter <R[:ALPHA[:N0]]>: Smooths sparse counts before the\n"
    "     image is made: a pixel's counts are spread over a radius that\n"
    "     shrinks from R (1 to 8) as its count grows from N0 (default 1),\n"
    "     as (R/r)^(1/ALPHA) (ALPHA from 1/16 to 4, default 0.5).\n"
    "  --equalize: Equalizes the image: a pixel's brightness is the share of\n"
    "     the nonzero pixels that are no brighter than it, rather than its\n"
    "     count over the largest count. -g applies to that share.\n"
    "  --local-equalize <TX[xTY][:CLIP]>: Equalizes the image tile by tile:\n"
    "     the image is cut into TX by TY tiles (1 to 16 a side, TY = TX\n"
    "     if left out), every tile gets the curve of --equalize over its\n"
    "     own pixels, and a pixel the blend of the curves of the four tile\n"
    "     centres around it. CLIP (0 = off, or 1 to 256; default 4) limits\n"
    "     how far a tile may raise its contrast over an even spread.\n"
    "\n"
    "The following settings control the location of the output image on the\n"
    "complex plane, but samples are always drawn from the entire Mandelbrot-\n"
    "set domain (-2-2i to 2+2i). So these settings can be used to save\n"
    "memory or \"crop\" the output, but won't otherwise speed up rendering:\n"
    "  --min-real <min real>: The minimum value along the real axis to\n"
    "             include in the output image. Defaults to -2.0.\n"
    "  --max-real <max real>: The maximum value along the real axis to\n"
    "             include in the output image. Defaults to 2.0.\n"
    "  --min-imag <min imag>: The minimum value along the imaginary axis to\n"
    "             include in the output image. Defaults to -2.0.\n"
    "  --max-imag <max imag>: The maximum value along the imaginary axis to\n"
    "             include in the output image. Defaults to 2.0.\n";

// Usage always ends the process with status 0, also after a bad argument (cudabrot.cu:619).
[[noreturn]] void usage_and_exit(const char *program) {
  printf("Usage: %s [options]\n\n", program);
  fputs(kUsageBody, stdout);
  exit(0);
}

// ---- argument table ----------------------------------------------------------------------------

enum class Value { kNone, kInt, kLong, kDouble, kText };  // kInt: truncated to int like the reference's flags

struct Flag {
  const char *name;
  Value value;
  const char *missing_value_message;  // nullptr: "Argument %s needs a value."
  bool revalidates_canvas;            // -w -h --min/max-*: canvas re-checked at once (:704-749)
  // stores the value; returns kOk, or the message of a bad value, printed as "<message>: <the value's text>"
  std::function<const char *(Settings &, long, double, const char *)> store;
};
const char *const kOk = nullptr;

#define CB_TEXT_OF_(x) #x
#define CB_TEXT_OF(x) CB_TEXT_OF_(x)  // a macro's value as text, for a message

// The four rows of a cell-sourced render, --focus and --aim: FLAG, FLAG-level L, FLAG-probe PASSES, FLAG-dilate D into the
// CellFlags `member` of Settings, `word` what the messages call it.  Each value flag turns the render on.
#define CB_CELL_FLAGS(flag, word, member)                                                                     \
  {flag, Value::kNone, nullptr, false,                                                                        \
   [](Settings &s, long, double, const char *) { s.member.on = true; return kOk; }},                          \
  {flag "-level", Value::kInt, nullptr, false,                                                                \
   [](Settings &s, long i, double, const char *) {                                                            \
     s.member.on = true;                                                                                      \
     if (i < CB_FOCUS_MIN_LEVEL || i > CB_FOCUS_MAX_LEVEL) return "Invalid " word " level (want 4 to 10)";    \
     s.member.level = (int) i;                                                                                \
     return kOk;                                                                                              \
   }},                                                                                                        \
  {flag "-probe", Value::kInt, nullptr, false,                                                                \
   [](Settings &s, long i, double, const char *) {                                                            \
     s.member.on = true;                                                                                      \
     if (i < 1) return "Invalid " word " probe (want at least 1 pass)";                                       \
     s.member.probe = i;                                                                                      \
     return kOk;                                                                                              \
   }},                                                                                                        \
  {flag "-dilate", Value::kInt, nullptr, false,                                                               \
   [](Settings &s, long i, double, const char *) {                                                            \
     s.member.on = true;                                                                                      \
     if (i < 0) return "Invalid " word " dilation (want 0 or more cells)";                                    \
     s.member.dilate = (int) i;                                                                               \
     return kOk;                                                                                              \
   }},

const std::vector<Flag> &flag_table() {
  static const std::vector<Flag> table = {
      {"-d", Value::kInt, nullptr, false,
       [](Settings &s, long i, double, const char *) { s.device = (int) i; return kOk; }},
      {"-o", Value::kText, "Missing output file name.", false,
       [](Settings &s, long, double, const char *t) { s.output_image = t; return kOk; }},
      {"-s", Value::kText, "Missing in-progress buffer file name.", false,
       [](Settings &s, long, double, const char *t) { s.inprogress_file = t; return kOk; }},
      {"-m", Value::kInt, nullptr, false,
       [](Settings &s, long i, double, const char *) {
         s.iterations.max_escape_iterations = (int) i;
         if (s.iterations.max_escape_iterations > 60000) {  // cudabrot.cu:692-695
           printf("Warning: Using a high number of iterations may cause the "
                  "program respond slowly to Ctrl+C or time running out.\n");
         }
         return kOk;
       }},
      {"-c", Value::kInt, nullptr, false,
       [](Settings &s, long i, double, const char *) { s.iterations.min_escape_iterations = (int) i; return kOk; }},
      {"-w", Value::kInt, nullptr, true,
       [](Settings &s, long i, double, const char *) { s.canvas.w = (int) i; return kOk; }},
      {"-h", Value::kInt, nullptr, true,
       [](Settings &s, long i, double, const char *) { s.canvas.h = (int) i; return kOk; }},
      {"-g", Value::kDouble, nullptr, false,
       [](Settings &s, long, double d, const char *) { s.gamma_correction = d; return kOk; }},
      {"-t", Value::kDouble, nullptr, false,
       [](Settings &s, long, double d, const char *) { s.seconds_to_run = d; return kOk; }},
      {"--min-real", Value::kDouble, nullptr, true,
       [](Settings &s, long, double d, const char *) { s.canvas.min_real = d; return kOk; }},
      {"--max-real", Value::kDouble, nullptr, true,
       [](Settings &s, long, double d, const char *) { s.canvas.max_real = d; return kOk; }},
      {"--min-imag", Value::kDouble, nullptr, true,
       [](Settings &s, long, double d, const char *) { s.canvas.min_imag = d; return kOk; }},
      {"--max-imag", Value::kDouble, nullptr, true,
       [](Settings &s, long, double d, const char *) { s.canvas.max_imag = d; return kOk; }},
      // extensions, which the reference answers with its usage text
      // --passes N: the run length in reference passes, not by the clock
      {"--passes", Value::kInt, nullptr, false,
       [](Settings &s, long i, double, const char *) { s.fixed_passes = i < 0 ? 0 : i; return kOk; }},
      // --kernel simple|timed|full: a validation variant of the draw kernel (include/cudabrot_amd.h, CB_KERNEL_*)
      {"--kernel", Value::kText, nullptr, false,
       [](Settings &s, long, double, const char *t) {
         s.kernel_variant = (strcmp(t, "simple") == 0)  ? CB_KERNEL_SIMPLE
                            : (strcmp(t, "timed") == 0) ? CB_KERNEL_TIMED
                            : (strcmp(t, "full") == 0)  ? CB_KERNEL_FULL_ITERATE
                                                        : CB_KERNEL_DEFAULT;
         return kOk;
       }},
      // --stats: the counters of the run (and what defines a projected run) as JSON lines on stderr
      {"--stats", Value::kNone, nullptr, false,
       [](Settings &s, long, double, const char *) { s.print_stats = true; return kOk; }},
      // --channel MAX:MIN:FILE, up to CB_MAX_CHANNELS times: one image per iteration window from one fused render
      {"--channel", Value::kText, nullptr, false,
       [](Settings &s, long, double, const char *t) {
         int mx = 0, mn = 0, used = 0;
         if (s.n_channels >= CB_MAX_CHANNELS || sscanf(t, "%d:%d:%n", &mx, &mn, &used) < 2 || used == 0 ||
             t[used] == 0) {
           return "Invalid channel (want MAX:MIN:FILE, at most " CB_TEXT_OF(CB_MAX_CHANNELS) " of them)";
         }
         s.channel_window[s.n_channels] = {mx, mn};
         s.channel_file[s.n_channels] = t + used;
         s.n_channels++;
         return kOk;
       }},
      // --gpus N: the render sharded over devices -d .. -d + N - 1, summed once at the end
      {"--gpus", Value::kInt, nullptr, false,
       [](Settings &s, long i, double, const char *) { s.gpus = (i < 1) ? 1 : (i > 64 ? 64 : (int) i); return kOk; }},
      // --burning-ship: the reference's compile-time variant (cudabrot.cu:15-17) as a flag
      {"--burning-ship", Value::kNone, nullptr, false,
       [](Settings &s, long, double, const char *) { s.burning_ship = true; return kOk; }},
      // --anti: the anti-Buddhabrot, the orbits that never escape (include/cudabrot_amd.h, CB_KERNEL_FLAG_ANTI)
      {"--anti", Value::kNone, nullptr, false,
       [](Settings &s, long, double, const char *) { s.anti = true; return kOk; }},
      // --focus, --focus-level L, --focus-probe PASSES, --focus-dilate D: a cropped canvas sampled only from the cells of
      // the plane whose samples reach it (include/cudabrot_amd.h, "Focused render"); each value flag turns --focus on
      CB_CELL_FLAGS("--focus", "focus", focus)
      // --aim, --aim-level L, --aim-probe PASSES, --aim-dilate D: a cropped plotted render sampled only from the cells of its
      // sample plane whose samples reach the canvas (include/cudabrot_amd.h, "Aimed render"); each value flag turns --aim on
      CB_CELL_FLAGS("--aim", "aim", aim)
      // --project a,b,c,d:e,f,g,h, --plane X,Y, --rotate X,Y:DEG: the plane of the 4-D set (z_re, z_im, c_re, c_im) the
      // orbits are plotted on (include/cudabrot_amd.h, "Projected render")
      {"--project", Value::kText, nullptr, false,
       [](Settings &s, long, double, const char *t) {
         s.project_given = true;
         return parse_projection(t, s.projection) ? kOk : "Invalid projection (want a,b,c,d:e,f,g,h, eight finite numbers)";
       }},
      {"--plane", Value::kText, nullptr, false,
       [](Settings &s, long, double, const char *t) {
         const char *rest = nullptr;
         const int x = axis_of(t, ',', &rest);
         const int y = x < 0 ? -1 : axis_of(rest, 0, &rest);
         s.plane_given = true;
         if (x < 0 || y < 0 || x == y) return "Invalid plane (want X,Y, two different axes of zr, zi, cr, ci)";
         // the rotations start from the plane
         if (s.rotate_given) return "Invalid plane (--plane goes before the first --rotate)";
         for (int j = 0; j < 8; ++j) s.projection[j] = 0.0;
         s.projection[x] = 1.0;
         s.projection[4 + y] = 1.0;
         return kOk;
       }},
      {"--rotate", Value::kText, nullptr, false,
       [](Settings &s, long, double, const char *t) {
         s.rotate_given = true;
         if (s.project_given) return kOk;  // refused after parsing (the refusal table); the matrix given is not touched
         return rotate_projection(t, s.projection)
                    ? kOk
                    : "Invalid rotation (want X,Y:DEG, two different axes of zr, zi, cr, ci and a finite angle)";
       }},
      // --power D: the Multibrot step z^D + c, D = 3 .. 8, on the projected path (include/cudabrot_amd.h, "Multibrot
      // step"); text: a value that is no integer gets the flag's own message
      {"--power", Value::kText, nullptr, false,
       [](Settings &s, long, double, const char *t) {
         char *end = nullptr;
         const long d = strtol(t, &end, 10);
         if (t[0] == 0 || *end != 0 || d < CB_POWER_MIN || d > CB_POWER_MAX) {
           return "Invalid power (want an integer from 3 to 8)";
         }
         s.power = (int) d;
         return kOk;
       }},
      // --julia RE,IM: the Buddhabrot of the Julia set of c = RE + IM i: c fixed, the samples are the starting points;
      // with --power or --burning-ship, on any plane (include/cudabrot_amd.h, "Julia render")
      {"--julia", Value::kText, nullptr, false,
       [](Settings &s, long, double, const char *t) {
         s.julia = true;
         return parse_julia(t, s.julia_c) ? kOk : "Invalid julia parameter (want RE,IM, two numbers from -2 to 2)";
       }},
      // --phoenix RE,IM: the Phoenix step z^2 + c + p z_prev with p = RE + IM i, a step with memory, on the projected path
      // with any plane and with --julia (include/cudabrot_amd.h, "Phoenix render"); parsed as --julia's value is
      {"--phoenix", Value::kText, nullptr, false,
       [](Settings &s, long, double, const char *t) {
         s.phoenix = true;
         return parse_julia(t, s.phoenix_p) ? kOk : "Invalid phoenix parameter (want RE,IM, two numbers from -2 to 2)";
       }},
      // --bounded: the orbits that never escape, plotted on any plane under any step of the projected path, with --julia
      // too (include/cudabrot_amd.h, "Bounded render"): --anti's orbits on the plotted path
      {"--bounded", Value::kNone, nullptr, false,
       [](Settings &s, long, double, const char *) { s.bounded = true; return kOk; }},
      // --period-palette K:RRGGBB[,K:RRGGBB...]: the orbits of a --bounded render coloured by the period of the cycle they
      // fall onto: --palette's syntax with K a period, 0 the colour of the orbits without one; three planes of integer
      // weights, -o receives one 16-bit PPM (include/cudabrot_amd.h, "Period-palette render").  --period-eps X: the
      // tolerance of its return test (hexfloats accepted)
      {"--period-palette", Value::kText, nullptr, false,
       [](Settings &s, long, double, const char *t) {
         s.period_stops.n = parse_palette(t, s.period_stops.at);
         if (s.period_palette() && s.period_stops.at[s.period_stops.n - 1].k >= CB_PERIOD_MAX_ENTRIES) s.period_stops.n = 0;
         return s.period_palette() ? kOk
                                   : "Invalid period palette (want K:RRGGBB,... K ascending from 0 to 1023, at most 16 stops)";
       }},
      {"--period-eps", Value::kDouble, nullptr, false,
       [](Settings &s, long, double d, const char *) {
         s.period_eps_given = true;
         if (!(d >= 0.0) || !isfinite(d)) return "Invalid period eps (want a finite number, 0 or more)";
         s.period_eps = d;
         return kOk;
       }},
      // --palette K:RRGGBB[,K:RRGGBB...]: orbits coloured by their escape index: colour stops interpolated into a table of
      // -m entries, three planes of integer weights, -o receives a 16-bit PPM; on the projected path with any plane,
      // --power, --julia or --burning-ship (include/cudabrot_amd.h, "Palette render")
      {"--palette", Value::kText, nullptr, false,
       [](Settings &s, long, double, const char *t) {
         s.palette_stops.n = parse_palette(t, s.palette_stops.at);
         return s.palette() ? kOk : "Invalid palette (want K:RRGGBB,... K ascending, at most 16 stops)";
       }},
      // --formula NAME: another step of the quadratic family, on the projected path with any plane, --julia or --palette
      // (include/cudabrot_amd.h, "Formula step")
      {"--formula", Value::kText, nullptr, false,
       [](Settings &s, long, double, const char *t) {
         static const char *const kNames[CB_FORMULA_MAX] = {"tricorn", "celtic", "buffalo", "perpendicular",
                                                            "celtic-tricorn"};  // codes 1 .. CB_FORMULA_MAX
         for (int code = 1; code <= CB_FORMULA_MAX; ++code) {
           if (strcmp(t, kNames[code - 1]) == 0) {
             s.formula = code;
             s.formula_name = kNames[code - 1];
             return kOk;
           }
         }
         return "Invalid formula (want tricorn, celtic, buffalo, perpendicular or celtic-tricorn)";
       }},
      // --depth ROW:MIN:MAX[:N]: the 4-D set sliced along a third row into N planes, a section (N = 1) or a volume; on
      // the projected path with any plane, --power, --julia, --formula or --burning-ship; -o receives N PGMs back to back
      // (include/cudabrot_amd.h, "Depth render")
      {"--depth", Value::kText, nullptr, false,
       [](Settings &s, long, double, const char *t) {
         s.depth_given = true;
         return parse_depth(t, &s.depth)
                    ? kOk
                    : "Invalid depth (want ROW:MIN:MAX[:N], ROW an axis zr, zi, cr, ci or four numbers, MIN < MAX, N from 1 "
                      "to " CB_TEXT_OF(CB_DEPTH_MAX_SLICES) ")";
       }},
      // --depth-palette K:RRGGBB[,K:RRGGBB...]: the points of a --depth render coloured by their slice: --palette's
      // syntax with K a slice index, the stops interpolated into a table of N entries, three planes of integer weights
      // whatever N is, -o receives one 16-bit PPM (include/cudabrot_amd.h, "Depth-palette render")
      {"--depth-palette", Value::kText, nullptr, false,
       [](Settings &s, long, double, const char *t) {
         s.depth_palette_stops.n = parse_palette(t, s.depth_palette_stops.at);
         return s.depth_palette() ? kOk : "Invalid depth palette (want K:RRGGBB,... K ascending, at most 16 stops)";
       }},
      // --sweep X,Y:DEG0:DEG1:F: F frames of the plane as it stands after every --plane / --rotate / --project, rotated in
      // the (X, Y) coordinate plane from DEG0 to DEG1 (exclusive), from ONE orbit pass; F planes, -o receives F PGMs back
      // to back with one common exposure (include/cudabrot_amd.h, "Frames render").  Applied last, wherever it stands.
      {"--sweep", Value::kText, nullptr, false,
       [](Settings &s, long, double, const char *t) {
         const bool again = s.sweep_given;
         s.sweep_given = true;
         return !again && parse_sweep(t, &s.sweep)
                    ? kOk
                    : "Invalid sweep (want X,Y:DEG0:DEG1:F, two different axes of zr, zi, cr, ci, two finite angles and 1 to "
                      CB_TEXT_OF(CB_FRAMES_MAX) " frames)";
       }},
      // --seed N: the generator's seed, 64 bits wide (rocrand_init)
      {"--seed", Value::kLong, nullptr, false,
       [](Settings &s, long i, double, const char *) { s.seed = (uint64_t) i; return kOk; }},
      // --rng-state FILE: the generator states beside the -s buffer, so that a resumed run continues the sample stream
      {"--rng-state", Value::kText, nullptr, false,
       [](Settings &s, long, double, const char *t) { s.rng_state_file = t; return kOk; }},
      // --state-format native|raw: raw is the -s file as the reference's bare buffer, uint32 when every count fits
      {"--state-format", Value::kText, nullptr, false,
       [](Settings &s, long, double, const char *t) {
         s.raw_state = strcmp(t, "raw") == 0;
         return s.raw_state || strcmp(t, "native") == 0 ? kOk : "Invalid state format (want native or raw)";
       }},
      // --color FILE, --compose rgb|hsl, --hue-shift X, --color-stretch B:W: the three --channel planes composed into one
      // 16-bit PPM (include/cudabrot_amd.h, "Colour image")
      {"--color", Value::kText, nullptr, false,
       [](Settings &s, long, double, const char *t) { s.color_file = t; return kOk; }},
      {"--compose", Value::kText, nullptr, false,
       [](Settings &s, long, double, const char *t) {
         if (strcmp(t, "rgb") == 0) {
           s.color.compose = CB_COMPOSE_RGB;
         } else if (strcmp(t, "hsl") == 0) {
           s.color.compose = CB_COMPOSE_HSL;
         } else {
           return "Invalid compose mode (want rgb or hsl)";
         }
         return kOk;
       }},
      {"--hue-shift", Value::kDouble, nullptr, false,
       [](Settings &s, long, double d, const char *) {
         if (!isfinite(d)) return "Invalid hue shift (want a finite number)";
         s.color.hue_shift = d;
         return kOk;
       }},
      {"--color-stretch", Value::kText, nullptr, false,
       [](Settings &s, long, double, const char *t) {
         // B:W, two numbers: B % of the pixels go black, W % white (finite, B >= 0, W >= 0, B + W < 100)
         char *end = nullptr;
         const double b = strtod(t, &end);
         bool ok = end != t && *end == ':';
         double w = 0.0;
         if (ok) {
           const char *rest = end + 1;
           w = strtod(rest, &end);
           ok = end != rest && *end == 0;
         }
         if (!(ok && isfinite(b) && isfinite(w) && b >= 0.0 && w >= 0.0 && b + w < 100.0)) {
           return "Invalid color stretch (want B:W, percentages with B + W < 100)";
         }
         s.color.black_percent = b;
         s.color.white_percent = w;
         return kOk;
       }},
      // --white-clip P: the white point of every image as a percentile of its lit counters (include/cudabrot_amd.h, "White
      // clip"); text: a value that is no number gets the flag's own message (hexfloats accepted)
      {"--white-clip", Value::kText, nullptr, false,
       [](Settings &s, long, double, const char *t) {
         char *end = nullptr;
         const double p = (t[0] == 0 || t[0] == ' ' || t[0] == '\t') ? NAN : strtod(t, &end);  // (strtod would skip blanks)
         if (!end || end == t || *end != 0 || !cb_white_clip_ok(p)) {
           return "Invalid white clip (want a percentage from 0 to below 100)";
         }
         s.white_clip = p;
         return kOk;
       }},
      // --density-filter R[:ALPHA[:N0]]: every image made from counters smoothed with a radius that falls as the count
      // rises (include/cudabrot_amd.h, "Density filter"); text, like the clip: R and N0 decimal digits, ALPHA in strtod's
      // syntax (hexfloats accepted); what cb_density_thresholds refuses is refused here
      {"--density-filter", Value::kText, nullptr, false,
       [](Settings &s, long, double, const char *t) {
         return parse_density(t, &s.density) ? kOk : "Invalid density filter (want R[:ALPHA[:N0]], R from 1 to 8)";
       }},
      // --equalize: every image exposed by the rank of its counters (include/cudabrot_amd.h, "Equalised image")
      {"--equalize", Value::kNone, nullptr, false,
       [](Settings &s, long, double, const char *) { s.equalize = true; return kOk; }},
      // --local-equalize TX[xTY][:CLIP]: every image exposed by the rank of its counters within the tiles of a grid
      // (include/cudabrot_amd.h, "Locally equalised image"); text: TX and TY decimal digits, CLIP in strtod's syntax
      // (hexfloats accepted), rounded to 1/256
      {"--local-equalize", Value::kText, nullptr, false,
       [](Settings &s, long, double, const char *t) {
         return parse_local_equalize(t, &s.local_equalize)
                    ? kOk
                    : "Invalid local equalisation (want TX[xTY][:CLIP], 1 to 16 tiles a side, CLIP 0 or from 1 to 256)";
       }},
      // --tonemap lut|thresholds|host: the form of the device tone map, or the reference's host loop
      {"--tonemap", Value::kText, nullptr, false,
       [](Settings &s, long, double, const char *t) {
         s.host_tonemap = strcmp(t, "host") == 0;
         s.tone_mode = (strcmp(t, "lut") == 0)          ? CB_TONE_LUT
                       : (strcmp(t, "thresholds") == 0) ? CB_TONE_THRESHOLDS
                                                        : CB_TONE_AUTO;
         return kOk;
       }},
  };
  return table;
}

// ---- refusal table -----------------------------------------------------------------------------

// What a render of its own may not be combined with: a predicate and the name it is refused by.
struct Partner {
  bool (*present)(const Settings &);
  const char *name;
};
const Partner kPower = {[](const Settings &s) { return s.power != 0; }, "--power"};
const Partner kShip = {[](const Settings &s) { return s.burning_ship; }, "--burning-ship"};
const Partner kAnti = {[](const Settings &s) { return s.anti; }, "--anti"};
const Partner kFocus = {[](const Settings &s) { return s.focus.on; }, "--focus"};
const Partner kChannel = {[](const Settings &s) { return s.n_channels > 0 || s.color_file; }, "--channel"};
const Partner kGpus = {[](const Settings &s) { return s.gpus > 1; }, "--gpus above 1"};
const Partner kRaw = {[](const Settings &s) { return s.raw_state; }, "--state-format raw"};
const Partner kPalette = {[](const Settings &s) { return s.palette(); }, "--palette"};
const Partner kDepth = {[](const Settings &s) { return s.depth_given; }, "--depth"};
const Partner kDepthPalette = {[](const Settings &s) { return s.depth_palette(); }, "--depth-palette"};
const Partner kFormula = {[](const Settings &s) { return s.formula != 0; }, "--formula"};
const Partner kSweep = {[](const Settings &s) { return s.sweep_given; }, "--sweep"};
const Partner kPhoenix = {[](const Settings &s) { return s.phoenix; }, "--phoenix"};
const Partner kPeriodPalette = {[](const Settings &s) { return s.period_palette(); }, "--period-palette"};
const Partner kColor = {[](const Settings &s) { return s.color_file != nullptr; }, "--color"};
const Partner kWhiteClip = {[](const Settings &s) { return s.white_clip > 0.0; }, "--white-clip"};
const Partner kEqualize = {[](const Settings &s) { return s.equalize; }, "--equalize"};

// The refusals behind the flag loop, in the order they are looked at: the first row that applies and has something to
// say ends the process.  A row says "<subject> does not combine with <the first of its partners that is present>.", or,
// where it has no partners, a message of its own.  The order of the rows and of each row's partners is observable
// (tests/test_cli_refusals.py) and is each row's own.
struct Refusal {
  bool (*applies)(const Settings &);
  const char *subject;
  std::vector<Partner> partners;
  void (*say)(const Settings &);
};

const std::vector<Refusal> &refusal_table() {
  static const std::vector<Refusal> table = {
      // an aimed render is a projected, Julia or bounded render of one plane without a table, drawn from a cell list
      // (include/cudabrot_amd.h, "Aimed render").  The first row: it combines with --bounded, --formula, --power, --julia and
      // a projection, whose rows would otherwise say what it refuses in their own name -- and no line without --aim meets it
      {[](const Settings &s) { return s.aim.on; }, "--aim",
       {kFocus, kAnti, kPalette, kPeriodPalette, kDepth, kDepthPalette, kSweep, kPhoenix, kChannel, kGpus}, nullptr},
      // a period-palette render is a bounded render with a table (include/cudabrot_amd.h, "Period-palette render"): its
      // rows stand ahead of --bounded's, which refuses everything else in its own name -- and no line without the two flags
      // meets them
      {[](const Settings &s) { return s.period_eps_given && !s.period_palette(); }, nullptr, {},
       [](const Settings &) { printf("--period-eps needs --period-palette.\n"); }},
      {[](const Settings &s) { return s.period_palette() && !s.bounded; }, nullptr, {},
       [](const Settings &) { printf("--period-palette needs --bounded.\n"); }},
      {[](const Settings &s) { return s.period_palette(); }, "--period-palette", {kRaw}, nullptr},
      // a bounded render is a projected or Julia render, under any of their steps, that plots the other orbits into one
      // plane (include/cudabrot_amd.h, "Bounded render").  The first row: it combines with --formula, --power, --julia and
      // a projection, whose rows would otherwise say what it refuses in their own name -- and no line without --bounded
      // meets it
      {[](const Settings &s) { return s.bounded; }, "--bounded",
       {kAnti, kPalette, kDepth, kDepthPalette, kSweep, kPhoenix, kFocus, kChannel, kGpus}, nullptr},
      // a formula render is a projected render with a step of its own (include/cudabrot_amd.h, "Formula step"): its
      // refusals come before those of the palette, the Multibrot step, c and the projection, which it would otherwise trip
      {[](const Settings &s) { return s.formula != 0; }, "--formula", {kPower, kShip, kAnti, kFocus, kChannel, kGpus},
       nullptr},
      // a palette render is a projected render with three planes (include/cudabrot_amd.h, "Palette render"): its refusals
      // come before those of the step, of c and of the projection, which it would otherwise trip
      {[](const Settings &s) { return s.palette(); }, "--palette", {kAnti, kFocus, kChannel, kGpus, kRaw}, nullptr},
      {[](const Settings &s) {  // the table has -m entries
         return s.palette() && (s.iterations.max_escape_iterations < 1 ||
                                s.iterations.max_escape_iterations > CB_PALETTE_MAX_ENTRIES);
       },
       nullptr, {}, [](const Settings &) { printf("--palette needs -m from 1 to %d.\n", CB_PALETTE_MAX_ENTRIES); }},
      // a Multibrot render is a projected render with a step of its own (include/cudabrot_amd.h, "Multibrot step"): its
      // refusals come before the projection's, which it would otherwise trip
      {[](const Settings &s) { return s.power != 0; }, "--power", {kShip, kAnti, kFocus, kChannel, kGpus}, nullptr},
      // a Julia render is a projected render as well (include/cudabrot_amd.h, "Julia render"), with either step but the
      // Multibrot step's own refusals before its own
      {[](const Settings &s) { return s.julia; }, "--julia", {kAnti, kFocus, kChannel, kGpus}, nullptr},
      // a projected render is one plane of escaping orbits on one device, sampled uniformly (include/cudabrot_amd.h,
      // cb_renderer_set_projection)
      {[](const Settings &s) { return s.project_given && (s.plane_given || s.rotate_given); }, nullptr, {},
       [](const Settings &) { printf("--project does not combine with --plane or --rotate.\n"); }},
      {[](const Settings &s) { return s.projected(); }, "A projection", {kChannel, kAnti, kFocus, kGpus}, nullptr},
      // a focused render is one plane of escaping orbits on one device (include/cudabrot_amd.h, cb_renderer_set_focus);
      // with --gpus every rank would probe a mask of its own
      {[](const Settings &s) { return s.focus.on; }, "--focus", {kChannel, kAnti, kGpus}, nullptr},
      // no fused anti channels (include/cudabrot_amd.h)
      {[](const Settings &s) { return s.anti; }, "--anti", {kChannel}, nullptr},
      // after parsing: --color and the --channel flags come in any order
      {[](const Settings &s) { return s.color_file && s.n_channels != 3; }, nullptr, {},
       [](const Settings &s) { printf("--color needs exactly 3 --channel images, got %d.\n", s.n_channels); }},
      // a depth render is a projected render with N planes (include/cudabrot_amd.h, "Depth render"); behind every other
      // row: where a flag that turns the projected path on is given as well, that flag's row has spoken already
      {[](const Settings &s) { return s.depth_given; }, "--depth", {kPalette, kAnti, kFocus, kChannel, kGpus, kRaw}, nullptr},
      // a depth-palette render is a depth render with a table (include/cudabrot_amd.h, "Depth-palette render"): whatever
      // --depth refuses, its row above has refused
      {[](const Settings &s) { return s.depth_palette() && !s.depth_given; }, nullptr, {},
       [](const Settings &) { printf("--depth-palette needs --depth.\n"); }},
      // a frames render is a projected render with F planes (include/cudabrot_amd.h, "Frames render"); behind every older
      // row: where one of them refuses the line, that row has spoken already
      {[](const Settings &s) { return s.sweep_given; }, "--sweep",
       {kPalette, kDepth, kDepthPalette, kAnti, kFocus, kChannel, kGpus, kRaw}, nullptr},
      // a Phoenix render is a projected or Julia render with a step of its own and one plane (include/cudabrot_amd.h,
      // "Phoenix render"); the last row, likewise
      {[](const Settings &s) { return s.phoenix; }, "--phoenix",
       {kPower, kFormula, kShip, kPalette, kDepth, kDepthPalette, kSweep, kAnti, kFocus, kChannel, kGpus}, nullptr},
      // a white clip exposes the planes' images; the colour stage stretches them itself (include/cudabrot_amd.h, "White
      // clip").  The last row, likewise
      {[](const Settings &s) { return s.white_clip > 0.0; }, "--white-clip", {kColor}, nullptr},
      // the density filter makes 64-bit counters; the colour stage works on the planes' 16-bit images
      // (include/cudabrot_amd.h, "Density filter").  The last row, likewise
      {[](const Settings &s) { return s.density.radius > 0; }, "--density-filter", {kColor}, nullptr},
      // an equalised image has an exposure of its own: no white point to clip against, and the colour stage stretches its
      // planes itself (include/cudabrot_amd.h, "Equalised image").  The last row, likewise
      {[](const Settings &s) { return s.equalize; }, "--equalize", {kWhiteClip, kColor}, nullptr},
      // a locally equalised image is cut into tiles of at least a pixel (-w and -h may stand behind the flag), and is an
      // exposure of its own as the equalised one is (include/cudabrot_amd.h, "Locally equalised image").  The last rows,
      // likewise
      {[](const Settings &s) {
         return s.local_equalize.tx > 0 && (s.local_equalize.tx > s.canvas.w || s.local_equalize.ty > s.canvas.h);
       },
       nullptr, {}, [](const Settings &s) {
         printf("--local-equalize needs a pixel per tile: %dx%d tiles on a %dx%d image.\n", s.local_equalize.tx,
                s.local_equalize.ty, s.canvas.w, s.canvas.h);
       }},
      {[](const Settings &s) { return s.local_equalize.tx > 0; }, "--local-equalize", {kEqualize, kWhiteClip, kColor}, nullptr},
  };
  return table;
}

// Canvas validation with the reference's messages (cudabrot.cu:505-527).
bool canvas_ok(Settings &s) {
  const char *why = nullptr;
  if (cb_recompute_pixel_deltas(&s.canvas, &why)) return true;
  printf("%s\n", why);
  return false;
}

}  // namespace

Settings parse_arguments(int argc, char **argv) {
  Settings s;
  if (!canvas_ok(s)) {  // cudabrot.cu:539-542
    printf("Internal error setting default canvas boundaries!\n");
    exit(1);
  }
  for (int i = 1; i < argc; i++) {
    const char *arg = argv[i];
    if (strcmp(arg, "--help") == 0) usage_and_exit(argv[0]);
    const Flag *flag = nullptr;
    for (const Flag &f : flag_table()) {
      if (strcmp(arg, f.name) == 0) {
        flag = &f;
        break;
      }
    }
    if (!flag) {
      printf("Invalid argument: %s\n", arg);  // cudabrot.cu:751
      usage_and_exit(argv[0]);
    }
    long as_int = 0;
    double as_double = 0.0;
    const char *text = nullptr;
    if (flag->value != Value::kNone) {
      if (i + 1 >= argc) {
        if (flag->missing_value_message) {
          printf("%s\n", flag->missing_value_message);
        } else {
          printf("Argument %s needs a value.\n", arg);  // cudabrot.cu:629,648
        }
        usage_and_exit(argv[0]);
      }
      text = argv[++i];
      if (flag->value != Value::kText) {
        // whole-string numbers only; an empty string is not a number (cudabrot.cu:632-639,651-656)
        char *end = nullptr;
        if (flag->value == Value::kInt) {
          as_int = (int) strtol(text, &end, 10);  // truncated to int like the reference
        } else if (flag->value == Value::kLong) {
          as_int = (long) strtoull(text, &end, 10);
        } else {
          as_double = strtod(text, &end);
        }
        if (*end != 0 || text[0] == 0) {
          printf("Invalid number given to argument %s: %s\n", arg, text);
          usage_and_exit(argv[0]);
        }
      }
    }
    if (const char *bad = flag->store(s, as_int, as_double, text)) {
      printf("%s: %s\n", bad, text);
      usage_and_exit(argv[0]);
    }
    if (flag->revalidates_canvas && !canvas_ok(s)) usage_and_exit(argv[0]);
  }
  for (const Refusal &row : refusal_table()) {
    if (!row.applies(s)) continue;
    if (row.say) {
      row.say(s);
      usage_and_exit(argv[0]);
    }
    for (const Partner &partner : row.partners) {
      if (partner.present(s)) {
        printf("%s does not combine with %s.\n", row.subject, partner.name);
        usage_and_exit(argv[0]);
      }
    }
  }
  return s;
}

}  // namespace cb
