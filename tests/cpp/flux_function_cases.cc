// CPU check of the function flux of the scalar conservation equation (flux_compile, flux_evaluate_points of
// ryujin_amd/csrc/expression.hpp) without the library around it.
//   flux_function_cases grammar    the variable u; x, t, pi, rand, an assignment, unbalanced parentheses and text behind
//                                  a component, each with its status and the character position in the WHOLE string
//   flux_function_cases components the component count against dim = 1, 2, 3: too few, too many, a trailing ';', ";;",
//                                  the empty string
//   flux_function_cases limits     RYUJIN_EXPR_MAX_INSTRUCTIONS instructions and RYUJIN_EXPR_MAX_STACK operands PER
//                                  COMPONENT are accepted, one more of either is refused, in the last component too
//   flux_function_cases values     Horner polynomials, Buckley-Leverett and a kinked flux against the same operations
//                                  written out here, bit for bit; the gradient (f(u + d) - f(u - d)) / (2 * d); n = 0 and
//                                  gradient = NULL
// Exit status 0 and "ok", or one line per failure and status 1.
// (test infrastructure; built by tests/test_flux_function_cpu.py)
#include <cmath>
#include <cstdio>
#include <cstring>
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

  std::unique_ptr<FluxProgram> program = std::make_unique<FluxProgram>();

  void accepted(const std::string &expression, const int dim, const int n_instructions = -1)
  {
    std::string error;
    const int status = flux_compile(expression.c_str(), dim, *program, error);
    if (status != kExprOk) {
      std::printf("'%.60s' (dim %d): status %d (%s)\n", expression.c_str(), dim, status, error.c_str());
      ++failures;
    } else if (n_instructions >= 0 && (program->n_instructions != n_instructions || program->n != n_instructions + dim)) {
      std::printf("'%.60s' (dim %d): %d instructions and %d with the closers, expected %d\n", expression.c_str(), dim,
                  program->n_instructions, program->n, n_instructions);
      ++failures;
    }
  }

  void refused(const std::string &expression, const int dim, const int status, const long position)
  {
    std::string error;
    const int got = flux_compile(expression.c_str(), dim, *program, error);
    const std::string needle = "at character " + std::to_string(position) + " ";
    if (got != status || (position >= 0 && error.find(needle) == std::string::npos)) {
      std::printf("'%.60s' (dim %d): status %d (%.200s), expected %d at character %ld\n", expression.c_str(), dim, got,
                  error.c_str(), status, position);
      ++failures;
    }
  }

  void grammar()
  {
    accepted("u", 1, 1);
    accepted(" u ; u*u ", 2, 4);
    accepted("sin(u); cos(u); if(u < 0.5, u, 1 - u)", 3);
    accepted("u*u/(u*u + 0.25*(1-u)*(1-u))", 1);
    refused("x", 1, kExprErrArg, 0);
    refused("u + t", 1, kExprErrArg, 4);
    refused("u; u + y", 2, kExprErrArg, 7);
    refused("u; z", 3, kExprErrArg, -1); /* (two components in 3-D: the count comes first) */
    refused("u; u; z", 3, kExprErrArg, 6);
    refused("pi * u", 1, kExprErrArg, 0);
    refused("u; rand()", 2, kExprErrUnsupported, 3);
    refused("u = 3", 1, kExprErrUnsupported, 2);
    refused("u; v = u", 2, kExprErrArg, 3); /* (the unknown identifier v comes first) */
    refused("u; u = 1", 2, kExprErrUnsupported, 5);
    refused("(u + 1", 1, kExprErrArg, 0);
    refused("u; (u + 1", 2, kExprErrArg, 3);
    refused("u + 1)", 1, kExprErrArg, 5);
    refused("u; u + 1)", 2, kExprErrArg, 8);
    refused("u u", 1, kExprErrArg, 2);
    refused("u; u 2", 2, kExprErrArg, 5);
    refused("u; \"u\"", 2, kExprErrUnsupported, 3);
    std::string error;
    if (flux_compile(nullptr, 1, *program, error) != kExprErrArg) {
      std::printf("a null string is not refused\n");
      ++failures;
    }
    refused("u", 0, kExprErrArg, -1);
    refused("u", 4, kExprErrArg, -1);
  }

  void components()
  {
    /* the empty string: one empty component */
    refused("", 1, kExprErrArg, 0);
    refused("", 2, kExprErrArg, 0);
    refused("", 3, kExprErrArg, 0);
    refused("  ", 1, kExprErrArg, 2);
    /* too few: the position is the end of the string */
    refused("u", 2, kExprErrArg, 1);
    refused("u", 3, kExprErrArg, 1);
    refused("u; u", 3, kExprErrArg, 4);
    /* too many: the position is the first ';' too many */
    refused("u; u", 1, kExprErrArg, 1);
    refused("u; u; u", 1, kExprErrArg, 1);
    refused("u; u; u", 2, kExprErrArg, 4);
    refused("u; u; u; u", 3, kExprErrArg, 7);
    refused("u;u;u;u;u;u", 3, kExprErrArg, 5);
    /* a trailing ';' */
    refused("u;", 1, kExprErrArg, 1);
    refused("u;", 2, kExprErrArg, 2);  /* the empty second component */
    refused("u; ", 2, kExprErrArg, 3);
    refused("u; u;", 2, kExprErrArg, 4);
    refused("u; u;", 3, kExprErrArg, 5);
    /* ";;" */
    refused(";;", 1, kExprErrArg, 0);
    refused(";;", 2, kExprErrArg, 1);
    refused(";;", 3, kExprErrArg, 0); /* the empty first component */
    refused("u;;u", 3, kExprErrArg, 2);
    refused("u;u;", 3, kExprErrArg, 4);
    accepted("u;u;u", 3, 3);
    accepted("u;u", 2, 2);
  }

  /* 1+(1+( ... (1+1))) with `operands` ones: all of them are alive before the first addition */
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

  /* -u+1+ ... +1: `terms` operands, terms - 1 additions and the sign: 2 terms instructions */
  std::string left_sum(const int terms)
  {
    std::string s = "-u";
    for (int q = 1; q < terms; ++q)
      s += "+1";
    return s;
  }

  void limits()
  {
    const std::string longest = left_sum(RYUJIN_EXPR_MAX_INSTRUCTIONS / 2);
    const std::string deepest = right_nested_sum(RYUJIN_EXPR_MAX_STACK);
    accepted(longest, 1, RYUJIN_EXPR_MAX_INSTRUCTIONS);
    /* the limit holds per component: three full components */
    accepted(longest + ";" + longest + ";" + longest, 3, 3 * RYUJIN_EXPR_MAX_INSTRUCTIONS);
    if (failures == 0) {
      const double u = 0.25;
      double value[3];
      flux_evaluate_points(*program, 3, 1e-10, &u, 1, value, nullptr);
      for (int d = 0; d < 3; ++d)
        if (value[d] != -0.25 + (RYUJIN_EXPR_MAX_INSTRUCTIONS / 2 - 1)) {
          std::printf("three full components: value %g in direction %d\n", value[d], d);
          ++failures;
        }
    }
    refused("-" + longest, 1, kExprErrArg, -1);
    refused(longest + ";-" + longest, 2, kExprErrArg, -1);
    refused("u;u;-" + longest, 3, kExprErrArg, -1);
    accepted(deepest, 1);
    accepted("u;" + deepest, 2);
    if (failures == 0) {
      const double u = 0.5;
      double value[2];
      flux_evaluate_points(*program, 2, 1e-10, &u, 1, value, nullptr);
      if (value[0] != 0.5 || value[1] != (double)RYUJIN_EXPR_MAX_STACK) {
        std::printf("%d operands: values %g %g\n", RYUJIN_EXPR_MAX_STACK, value[0], value[1]);
        ++failures;
      }
    }
    refused(right_nested_sum(RYUJIN_EXPR_MAX_STACK + 1), 1, kExprErrArg, -1);
    refused("u;" + right_nested_sum(RYUJIN_EXPR_MAX_STACK + 1), 2, kExprErrArg, -1);
    refused("u;" + std::string(100000, '(') + "1", 2, kExprErrArg, -1);
    refused(std::string(100000, '-') + "u", 1, kExprErrArg, -1);
  }

  /* the expected values: the same operations in the same order, on arguments the compiler cannot fold */
  double horner(const double (&c)[4], const double u)
  {
    return c[0] + u * (c[1] + u * (c[2] + u * c[3]));
  }
  double buckley_leverett(const double u)
  {
    return u * u / (u * u + 0.25 * (1. - u) * (1. - u));
  }
  double kinked(const double u)
  {
    return u < 0.5 ? u : 1. - u;
  }

  void values()
  {
    const char *expression = "0.5 + u*(-1.25 + u*(0.75 + u*0.125)); u*u/(u*u + 0.25*(1-u)*(1-u)); if(u < 0.5, u, 1 - u)";
    accepted(expression, 3);
    if (failures)
      return;
    const double c[4] = {0.5, -1.25, 0.75, 0.125};
    volatile double delta_seed = 1e-10;
    const double delta = delta_seed;
    std::vector<double> u;
    for (int q = 0; q < 1000; ++q)
      u.push_back(-2. + 4. * ((q * 7919) % 1000) / 1000. + 1. / 3.);
    u.push_back(0.5); /* the kink */
    u.push_back(0.5 - delta);
    u.push_back(0.);
    const size_t n = u.size();
    std::vector<double> value(3 * n, 7.), gradient(3 * n, 7.), value_only(3 * n, 7.);
    flux_evaluate_points(*program, 3, delta, u.data(), n, value.data(), gradient.data());
    flux_evaluate_points(*program, 3, delta, u.data(), n, value_only.data(), nullptr);
    for (size_t i = 0; i < n; ++i) {
      const double x = u[i];
      const double f[3] = {horner(c, x), buckley_leverett(x), kinked(x)};
      const double df[3] = {(horner(c, x + delta) - horner(c, x - delta)) / (2 * delta),
                            (buckley_leverett(x + delta) - buckley_leverett(x - delta)) / (2 * delta),
                            (kinked(x + delta) - kinked(x - delta)) / (2 * delta)};
      for (int d = 0; d < 3; ++d)
        if (!same_bits(value[3 * i + d], f[d]) || !same_bits(gradient[3 * i + d], df[d]) ||
            !same_bits(value_only[3 * i + d], f[d])) {
          std::printf("u = %.17g, direction %d: f %.17g (expected %.17g), df %.17g (expected %.17g)\n", x, d,
                      value[3 * i + d], f[d], gradient[3 * i + d], df[d]);
          ++failures;
        }
    }
    /* n = 0 writes nothing and reads nothing */
    double guard[2] = {7., 7.};
    flux_evaluate_points(*program, 3, delta, nullptr, 0, guard, guard + 1);
    if (guard[0] != 7. || guard[1] != 7.) {
      std::printf("n = 0 wrote something\n");
      ++failures;
    }
    /* a different operation order may differ in the last bit and must not crash */
    accepted("0.5*u*u", 1, 5);
    std::vector<double> a(n), b(n);
    flux_evaluate_points(*program, 1, delta, u.data(), n, a.data(), nullptr);
    accepted("u*0.5*u", 1, 5);
    flux_evaluate_points(*program, 1, delta, u.data(), n, b.data(), nullptr);
    for (size_t i = 0; i < n; ++i)
      if (!(std::fabs(a[i] - b[i]) <= 2.3e-16 * std::fabs(a[i]))) {
        std::printf("0.5*u*u and u*0.5*u differ by more than an ulp at u = %.17g\n", u[i]);
        ++failures;
      }
  }
} // namespace

int main(int argc, char **argv)
{
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "grammar")
    grammar();
  else if (mode == "components")
    components();
  else if (mode == "limits")
    limits();
  else if (mode == "values")
    values();
  else {
    std::printf("usage: flux_function_cases grammar|components|limits|values\n");
    return 2;
  }
  if (failures == 0)
    std::printf("ok\n");
  return failures == 0 ? 0 : 1;
}
