// CPU check of the function equation of state of EulerAEOS (eos_compile, eos_evaluate_points of
// ryujin_amd/csrc/expression.hpp) without the library around it.
//   eos_function_cases grammar   the variable sets: rho and e in pressure, temperature and speed of sound, rho and p in
//                                the specific internal energy; the wrong second variable, x, t, u, Euler's number
//                                without its underscore in the sie program, each with its status, the parameter's name
//                                and the character position within that string; 1e-3*e, 2*e, rho*e lex as literal times
//                                variable; _e is the constant
//   eos_function_cases limits    RYUJIN_EXPR_MAX_INSTRUCTIONS instructions and RYUJIN_EXPR_MAX_STACK operands PER
//                                EXPRESSION are accepted (four full programs), one more of either is refused; the
//                                recorded offsets
//   eos_function_cases defaults  NULL strings give the reference's defaults; non-finite interpolation parameters
//   eos_function_cases values    a stiffened gas and an if() equation of state against the same operations written out
//                                here, bit for bit; the round trip p(rho, sie(rho, p)) of these test expressions; n = 0
// Exit status 0 and "ok", or one line per failure and status 1.
// (test infrastructure; built by tests/test_eos_function_cpu.py, there also once with -fsanitize=address,undefined)
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include <string>
#include <vector>

#include "expression.hpp"

using namespace ryujin_hip;

namespace
{
  int failures = 0;

  bool same_bits(const double a, const double b)
  {
    return std::memcmp(&a, &b, sizeof(double)) == 0;
  }

  std::unique_ptr<EosProgram> program = std::make_unique<EosProgram>();

  /* `expression` as function `which`, the other three at their defaults */
  int compile_one(const int which, const char *expression, std::string &error)
  {
    const char *expressions[kEosPrograms] = {nullptr, nullptr, nullptr, nullptr};
    expressions[which] = expression;
    return eos_compile(expressions, 0., 0., 0., *program, error);
  }

  void accepted(const int which, const std::string &expression, const int n_instructions = -1)
  {
    std::string error;
    const int status = compile_one(which, expression.c_str(), error);
    if (status != kExprOk) {
      std::printf("%s '%.60s': status %d (%s)\n", eos_function_name(which), expression.c_str(), status, error.c_str());
      ++failures;
    } else if (n_instructions >= 0 && program->n_instructions(which) != n_instructions) {
      std::printf("%s '%.60s': %d instructions, expected %d\n", eos_function_name(which), expression.c_str(),
                  program->n_instructions(which), n_instructions);
      ++failures;
    }
  }

  void refused(const int which, const std::string &expression, const int status, const long position)
  {
    std::string error;
    const int got = compile_one(which, expression.c_str(), error);
    const std::string needle = "at character " + std::to_string(position) + " ";
    const std::string name = std::string("eos: ") + eos_function_name(which) + ": ";
    if (got != status || (position >= 0 && error.find(needle) == std::string::npos) || error.find(name) != 0) {
      std::printf("%s '%.60s': status %d (%.200s), expected %d at character %ld\n", eos_function_name(which),
                  expression.c_str(), got, error.c_str(), status, position);
      ++failures;
    }
  }

  double value_of(const int which, const double rho, const double second)
  {
    double out = 7.;
    eos_evaluate_points(*program, which, &rho, &second, 1, &out);
    return out;
  }

  void expect(const char *what, const double got, const double want)
  {
    if (!same_bits(got, want)) {
      std::printf("%s: %.17g, expected %.17g\n", what, got, want);
      ++failures;
    }
  }

  void grammar()
  {
    for (const int w : {kEosPressure, kEosTemperature, kEosSpeedOfSound}) {
      accepted(w, "rho*e", 3);
      accepted(w, " rho + e ", 3);
      refused(w, "rho*p", kExprErrArg, 4);
      refused(w, "p", kExprErrArg, 0);
    }
    accepted(kEosSpecificInternalEnergy, "p/rho", 3);
    refused(kEosSpecificInternalEnergy, "rho*e", kExprErrArg, 4);
    refused(kEosSpecificInternalEnergy, "e", kExprErrArg, 0);
    for (int w = 0; w < kEosPrograms; ++w) {
      refused(w, "x", kExprErrArg, 0);
      refused(w, "rho + t", kExprErrArg, 6);
      refused(w, "rho*u", kExprErrArg, 4);
      refused(w, "rho*y + z", kExprErrArg, 4);
      refused(w, "pi*rho", kExprErrArg, 0);
      refused(w, "rho*rand()", kExprErrUnsupported, 4);
      refused(w, "rho = 3", kExprErrUnsupported, 4);
      refused(w, "(rho + 1", kExprErrArg, 0);
      refused(w, "rho + 1)", kExprErrArg, 7);
      refused(w, "rho 2", kExprErrArg, 4);
      refused(w, "", kExprErrArg, 0);
      refused(w, "Rho", kExprErrArg, 0);
    }
    /* a literal's exponent needs digits: e behind a number is the variable */
    volatile double rho_seed = 1.75, e_seed = 2.5;
    const double rho = rho_seed, e = e_seed;
    accepted(kEosPressure, "1e-3*e", 3);
    expect("1e-3*e", value_of(kEosPressure, rho, e), 1e-3 * e);
    accepted(kEosPressure, "2*e", 3);
    expect("2*e", value_of(kEosPressure, rho, e), 2 * e);
    accepted(kEosPressure, "rho*e", 3);
    expect("rho*e", value_of(kEosPressure, rho, e), rho * e);
    accepted(kEosPressure, "2e1*e + 1.5E+1*rho", 7);
    expect("2e1*e + 1.5E+1*rho", value_of(kEosPressure, rho, e), 2e1 * e + 1.5E+1 * rho);
    refused(kEosPressure, "2e", kExprErrArg, 1); /* the literal 2, then text behind the expression */
    refused(kEosPressure, "2 e", kExprErrArg, 2);
    /* _e stays Euler's number, in every program */
    accepted(kEosPressure, "_e*e", 3);
    expect("_e*e", value_of(kEosPressure, rho, e), 2.718281828459045235360287 * e);
    accepted(kEosSpecificInternalEnergy, "_e*p + _pi", 5);
    expect("_e*p + _pi", value_of(kEosSpecificInternalEnergy, rho, e),
           2.718281828459045235360287 * e + 3.141592653589793238462643);
    refused(kEosSpecificInternalEnergy, "p*e", kExprErrArg, 2);
  }

  std::string right_nested_sum(const int operands)
  {
    std::string s;
    for (int q = 1; q < operands; ++q)
      s += "1+(";
    s += "1";
    for (int q = 1; q < operands; ++q)
      s += ")";
    return s;
  }

  /* -rho+1+ ... +1: 2 terms instructions */
  std::string left_sum(const int terms)
  {
    std::string s = "-rho";
    for (int q = 1; q < terms; ++q)
      s += "+1";
    return s;
  }

  void limits()
  {
    const std::string longest = left_sum(RYUJIN_EXPR_MAX_INSTRUCTIONS / 2);
    const std::string deepest = right_nested_sum(RYUJIN_EXPR_MAX_STACK);
    /* the limits hold per expression: four full programs back to back */
    const char *full[kEosPrograms] = {longest.c_str(), longest.c_str(), longest.c_str(), longest.c_str()};
    std::string error;
    if (eos_compile(full, 0., 0., 0., *program, error) != kExprOk) {
      std::printf("four full programs: %s\n", error.c_str());
      ++failures;
    } else {
      for (int w = 0; w <= kEosPrograms; ++w)
        if (program->offset[w] != w * RYUJIN_EXPR_MAX_INSTRUCTIONS) {
          std::printf("offset[%d] = %d\n", w, program->offset[w]);
          ++failures;
        }
      for (int w = 0; w < kEosPrograms; ++w)
        expect("a full program", value_of(w, 0.25, 3.), -0.25 + (RYUJIN_EXPR_MAX_INSTRUCTIONS / 2 - 1));
    }
    for (int w = 0; w < kEosPrograms; ++w) {
      refused(w, "-" + longest, kExprErrArg, -1);
      accepted(w, deepest);
      expect("the deepest program", value_of(w, 1., 1.), (double)RYUJIN_EXPR_MAX_STACK);
      refused(w, right_nested_sum(RYUJIN_EXPR_MAX_STACK + 1), kExprErrArg, -1);
      refused(w, std::string(100000, '(') + "1", kExprErrArg, -1);
      refused(w, std::string(100000, '-') + "rho", kExprErrArg, -1);
    }
    /* programs of different lengths: the offsets are the running sums */
    const char *mixed[kEosPrograms] = {"rho", "p/rho", "rho + e*e", nullptr};
    if (eos_compile(mixed, 0., 0., 0., *program, error) != kExprOk || program->offset[0] != 0 ||
        program->offset[1] != 1 || program->offset[2] != 4 || program->offset[3] != 9 ||
        program->offset[4] != 9 + program->n_instructions(kEosSpeedOfSound)) {
      std::printf("mixed programs: offsets %d %d %d %d %d (%s)\n", program->offset[0], program->offset[1],
                  program->offset[2], program->offset[3], program->offset[4], error.c_str());
      ++failures;
    } else {
      expect("program 0 of the mixed set", value_of(0, 3., 5.), 3.);
      expect("program 1 of the mixed set", value_of(1, 4., 6.), 1.5);
      expect("program 2 of the mixed set", value_of(2, 3., 5.), 28.);
    }
  }

  void defaults()
  {
    std::string error;
    if (eos_compile(nullptr, 0., 0., 0., *program, error) != kExprOk) {
      std::printf("the defaults: %s\n", error.c_str());
      ++failures;
      return;
    }
    volatile double rho_seed = 1.3, e_seed = 2.1, p_seed = 0.7;
    const double rho = rho_seed, e = e_seed, p = p_seed;
    expect("default pressure", value_of(kEosPressure, rho, e), (1.4 - 1.0) * rho * e);
    expect("default sie", value_of(kEosSpecificInternalEnergy, rho, p), p / (rho * (1.4 - 1.0)));
    expect("default temperature", value_of(kEosTemperature, rho, e), e / 718.);
    expect("default speed of sound", value_of(kEosSpeedOfSound, rho, e), std::sqrt(1.4 * (1.4 - 1.0) * e));
    /* one string given, the others NULL */
    const char *one[kEosPrograms] = {nullptr, "p", nullptr, nullptr};
    if (eos_compile(one, 0.1, 0.2, 0.3, *program, error) != kExprOk) {
      std::printf("one string: %s\n", error.c_str());
      ++failures;
    } else {
      expect("sie given", value_of(kEosSpecificInternalEnergy, rho, p), p);
      expect("pressure at its default", value_of(kEosPressure, rho, e), (1.4 - 1.0) * rho * e);
    }
    const double inf = std::numeric_limits<double>::infinity(), qnan = std::numeric_limits<double>::quiet_NaN();
    const double bad[6][3] = {{inf, 0., 0.}, {0., -inf, 0.}, {0., 0., inf}, {qnan, 0., 0.}, {0., qnan, 0.}, {0., 0., qnan}};
    const char *needle[3] = {"covolume b", "reference pressure", "reference specific internal energy"};
    for (int q = 0; q < 6; ++q) {
      error.clear();
      const int status = eos_compile(nullptr, bad[q][0], bad[q][1], bad[q][2], *program, error);
      if (status != kExprErrArg || error.find(needle[q % 3]) == std::string::npos) {
        std::printf("non-finite interpolation parameter %d: status %d (%s)\n", q, status, error.c_str());
        ++failures;
      }
    }
  }

  /* the expected values: the same operations in the same order, on arguments the compiler cannot fold */
  double stiffened_pressure(const double rho, const double e)
  {
    return (1.4 - 1.) * rho * (e - 0.1) / (1. - 0.05 * rho) - 1.4 * 0.5;
  }
  double stiffened_sie(const double rho, const double p)
  {
    return 0.1 + (p + 1.4 * 0.5) * (1. - 0.05 * rho) / (rho * (1.4 - 1.));
  }
  double kinked_pressure(const double rho, const double e)
  {
    return rho < 1. ? 0.4 * rho * e : 0.4 * rho * e + 0.25 * (rho - 1.);
  }
  double kinked_sie(const double rho, const double p)
  {
    return rho < 1. ? p / (0.4 * rho) : (p - 0.25 * (rho - 1.)) / (0.4 * rho);
  }

  void values()
  {
    std::vector<double> rho, e;
    for (int q = 0; q < 1000; ++q) {
      rho.push_back(0.2 + 2.8 * ((q * 7919) % 1000) / 1000. + 1. / 3000.);
      e.push_back(3. + 5. * ((q * 104729) % 1000) / 1000. + 1. / 7000.);
    }
    rho.push_back(1.); /* the kink */
    e.push_back(4.);
    const size_t n = rho.size();
    std::vector<double> p(n, 7.), back(n, 7.), again(n, 7.);
    std::string error;
    for (int set = 0; set < 2; ++set) {
      const char *expressions[kEosPrograms] = {
          set == 0 ? "(1.4 - 1.)*rho*(e - 0.1)/(1. - 0.05*rho) - 1.4*0.5"
                   : "if(rho < 1, 0.4*rho*e, 0.4*rho*e + 0.25*(rho - 1))",
          set == 0 ? "0.1 + (p + 1.4*0.5)*(1. - 0.05*rho)/(rho*(1.4 - 1.))"
                   : "if(rho < 1, p/(0.4*rho), (p - 0.25*(rho - 1))/(0.4*rho))",
          nullptr, nullptr};
      if (eos_compile(expressions, 0.05, 0.5, 0.1, *program, error) != kExprOk) {
        std::printf("set %d: %s\n", set, error.c_str());
        ++failures;
        continue;
      }
      eos_evaluate_points(*program, kEosPressure, rho.data(), e.data(), n, p.data());
      eos_evaluate_points(*program, kEosSpecificInternalEnergy, rho.data(), p.data(), n, back.data());
      eos_evaluate_points(*program, kEosPressure, rho.data(), back.data(), n, again.data());
      for (size_t i = 0; i < n; ++i) {
        const double want_p = set == 0 ? stiffened_pressure(rho[i], e[i]) : kinked_pressure(rho[i], e[i]);
        const double want_e = set == 0 ? stiffened_sie(rho[i], p[i]) : kinked_sie(rho[i], p[i]);
        if (!same_bits(p[i], want_p) || !same_bits(back[i], want_e)) {
          std::printf("set %d at (%.17g, %.17g): p %.17g (expected %.17g), e %.17g (expected %.17g)\n", set, rho[i],
                      e[i], p[i], want_p, back[i], want_e);
          ++failures;
        }
        /* the round trip of THESE expressions (the library checks no consistency): a handful of roundings of
         * well-conditioned operations; the stiffened gas subtracts 1.4 * 0.5 from a pressure of up to 12 */
        if (!(std::fabs(again[i] - p[i]) <= 64 * 2.3e-16 * (std::fabs(p[i]) + 0.7))) {
          std::printf("set %d at (%.17g, %.17g): round trip %.17g -> %.17g\n", set, rho[i], e[i], p[i], again[i]);
          ++failures;
        }
      }
    }
    /* n = 0 writes nothing and reads nothing */
    double guard = 7.;
    eos_evaluate_points(*program, kEosPressure, nullptr, nullptr, 0, &guard);
    if (guard != 7.) {
      std::printf("n = 0 wrote something\n");
      ++failures;
    }
  }
} // namespace

int main(int argc, char **argv)
{
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "grammar")
    grammar();
  else if (mode == "limits")
    limits();
  else if (mode == "defaults")
    defaults();
  else if (mode == "values")
    values();
  else if (mode == "all") {
    grammar();
    limits();
    defaults();
    values();
  } else {
    std::printf("usage: eos_function_cases grammar|limits|defaults|values|all\n");
    return 2;
  }
  if (failures == 0)
    std::printf("ok\n");
  return failures == 0 ? 0 : 1;
}
