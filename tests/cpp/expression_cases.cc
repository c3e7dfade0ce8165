// CPU check of the expression parser and interpreter (ryujin_amd/csrc/expression.hpp) without the library around it.
//   expression_cases grammar    values of the grammar table: precedence, associativity, rounding, the power rewrite,
//                               every function against <cmath> written out here
//   expression_cases refusals   every refusal with its status and the character position in the message
//   expression_cases limits     RYUJIN_EXPR_MAX_STACK operands and RYUJIN_EXPR_MAX_INSTRUCTIONS instructions are
//                               accepted, one more of either is refused; deep nesting is refused, not a stack overflow
// Exit status 0 and "ok", or one line per failure and status 1.
// (test infrastructure; built by tests/test_expression_cpu.py)
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>

#include "expression.hpp"

using namespace ryujin_hip;

namespace
{
  int failures = 0;

  bool same_bits(const double a, const double b)
  {
    return std::memcmp(&a, &b, sizeof(double)) == 0;
  }

  /* the value at (x, y, z, t) = (0.75, -1.25, 2.5, 0.5), dim = 3; read through a volatile so that the expected
   * values below come from the same run-time library as the interpreter's, not from the compiler's folding */
  volatile double seed[4] = {0.75, -1.25, 2.5, 0.5};
  const double X = seed[0], Y = seed[1], Z = seed[2], T = seed[3];

  void value(const char *expression, const double expected)
  {
    ExprProgram program;
    std::string error;
    const int status = expr_compile(expression, 3, program, error);
    if (status != kExprOk) {
      std::printf("'%s': status %d (%s)\n", expression, status, error.c_str());
      ++failures;
      return;
    }
    const double point[3] = {X, Y, Z};
    double out = 0.;
    expr_evaluate_points(program, 3, point, 1, T, &out);
    if (!same_bits(out, expected)) {
      std::printf("'%s': %.17g, expected %.17g\n", expression, out, expected);
      ++failures;
    }
  }

  void refused(const char *expression, const int dim, const int status, const int position)
  {
    ExprProgram program;
    std::string error;
    const int got = expr_compile(expression, dim, program, error);
    const std::string needle = "at character " + std::to_string(position) + " ";
    if (got != status || error.find(needle) == std::string::npos) {
      std::printf("'%s': status %d (%s), expected %d at character %d\n", expression, got, error.c_str(), status,
                  position);
      ++failures;
    }
  }

  void grammar()
  {
    value("2+3*4", 14.);
    value("2^3^2", 512.);
    value("-2^2", -4.);
    value("1 < 2 == 1", 1.);
    value("0 || 2 && 0", 0.);
    value("1 ? 2 : 3 ? 4 : 5", 2.);
    value("0 ? 2 : 0 ? 4 : 5", 5.);
    value("if(0.4,1,2)", 2.);
    value("if(0.5,1,2)", 1.);
    value("if(-0.5,1,2)", 1.);
    value("0.4 ? 1 : 2", 1.);
    value("0.4 | 0.3", 0.);
    value("0.4 || 0.3", 1.);
    value("0.6 & 1", 1.);
    value("int(2.5)", 3.);
    value("int(-2.5)", -3.);
    value("rint(2.5)", 3.);
    value("rint(-2.5)", -2.);
    value("min(3,1,2)", 1.);
    value("max(1)", 1.);
    value("max(1, 3, 2)", 3.);
    value("_pi", 3.14159265358979323846);
    value("_e", 2.71828182845904523536);
    value("1e-3", 1e-3);
    value(".5", .5);
    value("1.5E+2", 150.);
    value("  2 *\t( 3 + 4 )\n", 14.);
    value("2*-3", -6.);
    value("2^-1", 0.5);
    value("+x", X);
    value("7 - 2 - 1", 4.);
    value("8 / 4 / 2", 1.);
    value("x - y * z + t", X - Y * Z + T);
    value("(x - y) * (z + t)", (X - Y) * (Z + T));
    value("x^2", X * X);
    value("x^3", X * X * X);
    value("x^4", X * X * X * X);
    value("x^(2)", X * X);
    value("x^5", std::pow(X, 5.));
    value("pow(x,5)", std::pow(X, 5.));
    value("pow(x,2)", std::pow(X, 2.));
    value("x^2.5", std::pow(X, 2.5));
    value("x^t", std::pow(X, T));
    value("x <= 0.75", 1.);
    value("x >= 1", 0.);
    value("x != x", 0.);
    value("if(x < 0, sqrt(x), 3)", 3.); /* the NaN of the arm not taken is discarded */
    value("sign(y) + sign(0) + sign(z)", 0.);
    value("abs(y)", -Y);
    value("floor(y)", -2.);
    value("ceil(y)", -1.);
    value("sin(x)", std::sin(X));
    value("cos(x)", std::cos(X));
    value("tan(x)", std::tan(X));
    value("asin(x)", std::asin(X));
    value("acos(x)", std::acos(X));
    value("atan(x)", std::atan(X));
    value("sinh(x)", std::sinh(X));
    value("cosh(x)", std::cosh(X));
    value("tanh(x)", std::tanh(X));
    value("asinh(x)", std::asinh(X));
    value("acosh(z)", std::acosh(Z));
    value("atanh(x)", std::atanh(X));
    value("exp(x)", std::exp(X));
    value("log(x)", std::log(X));
    value("ln(x)", std::log(X));
    value("log2(x)", std::log2(X));
    value("log10(x)", std::log10(X));
    value("sqrt(x)", std::sqrt(X));
    value("cot(x)", 1. / std::tan(X));
    value("csc(x)", 1. / std::sin(X));
    value("sec(x)", 1. / std::cos(X));
    value("erf(x)", std::erf(X));
    value("erfc(x)", std::erfc(X));
    value("0.78539816339 * if(x*x + y*y < 1, 14, 1)", 0.78539816339 * 1.);
  }

  void refusals()
  {
    refused("rand(1)", 1, kExprErrUnsupported, 0);
    refused("1 + rand_seed(1)", 1, kExprErrUnsupported, 4);
    refused("sum(1,2)", 1, kExprErrUnsupported, 0);
    refused("avg(1,2)", 1, kExprErrUnsupported, 0);
    refused("max(\"a\", 1)", 1, kExprErrUnsupported, 4);
    refused("x = 3", 1, kExprErrUnsupported, 2);
    refused("x += 3", 1, kExprErrUnsupported, 3);
    refused("pi", 1, kExprErrArg, 0);
    refused("2 * foo", 1, kExprErrArg, 4);
    refused("foo(1)", 1, kExprErrArg, 0);
    refused("x + y", 1, kExprErrArg, 4);
    refused("x + z", 2, kExprErrArg, 4);
    refused("(1 + 2", 1, kExprErrArg, 0);
    refused("1 + 2)", 1, kExprErrArg, 5);
    refused("sin(1, 2)", 1, kExprErrArg, 0);
    refused("pow(1)", 1, kExprErrArg, 0);
    refused("if(1, 2)", 1, kExprErrArg, 0);
    refused("min()", 1, kExprErrArg, 0);
    refused("", 1, kExprErrArg, 0);
    refused("   ", 1, kExprErrArg, 3);
    refused("1 2", 1, kExprErrArg, 2);
    refused("1 +", 1, kExprErrArg, 3);
    refused("1 ? 2", 1, kExprErrArg, 5);
    refused("1e", 1, kExprErrArg, 1);
    refused("2 $ 3", 1, kExprErrArg, 2);
    refused("sin", 1, kExprErrArg, 0);
    refused("x", 0, kExprErrArg, 0);
    refused("x", 4, kExprErrArg, 0);
    ExprProgram program;
    std::string error;
    if (expr_compile(nullptr, 1, program, error) != kExprErrArg) {
      std::printf("a null string is not refused\n");
      ++failures;
    }
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

  /* -1+1+ ... +1: `ones` constants, ones - 1 additions and the sign: 2 ones instructions */
  std::string left_sum(const int ones)
  {
    std::string s = "-1";
    for (int q = 1; q < ones; ++q)
      s += "+1";
    return s;
  }

  void limits()
  {
    ExprProgram program;
    std::string error;
    const std::string deepest = right_nested_sum(RYUJIN_EXPR_MAX_STACK);
    if (expr_compile(deepest.c_str(), 1, program, error) != kExprOk || program.depth != RYUJIN_EXPR_MAX_STACK) {
      std::printf("%d operands: refused or depth %d (%s)\n", RYUJIN_EXPR_MAX_STACK, program.depth, error.c_str());
      ++failures;
    } else {
      const double point = 0.;
      double out = 0.;
      expr_evaluate_points(program, 1, &point, 1, 0., &out);
      if (out != (double)RYUJIN_EXPR_MAX_STACK) {
        std::printf("%d operands: value %g\n", RYUJIN_EXPR_MAX_STACK, out);
        ++failures;
      }
    }
    if (expr_compile(right_nested_sum(RYUJIN_EXPR_MAX_STACK + 1).c_str(), 1, program, error) != kExprErrArg ||
        error.find("at character ") == std::string::npos) {
      std::printf("%d operands are not refused (%s)\n", RYUJIN_EXPR_MAX_STACK + 1, error.c_str());
      ++failures;
    }

    const std::string longest = left_sum(RYUJIN_EXPR_MAX_INSTRUCTIONS / 2);
    if (expr_compile(longest.c_str(), 1, program, error) != kExprOk || program.n != RYUJIN_EXPR_MAX_INSTRUCTIONS) {
      std::printf("%d instructions: refused or %d (%s)\n", RYUJIN_EXPR_MAX_INSTRUCTIONS, program.n, error.c_str());
      ++failures;
    } else {
      const double point = 0.;
      double out = 0.;
      expr_evaluate_points(program, 1, &point, 1, 0., &out);
      if (out != (double)(RYUJIN_EXPR_MAX_INSTRUCTIONS / 2 - 2)) {
        std::printf("%d instructions: value %g\n", RYUJIN_EXPR_MAX_INSTRUCTIONS, out);
        ++failures;
      }
    }
    if (expr_compile(("-" + longest).c_str(), 1, program, error) != kExprErrArg ||
        error.find("at character ") == std::string::npos) {
      std::printf("%d instructions are not refused (%s)\n", RYUJIN_EXPR_MAX_INSTRUCTIONS + 1, error.c_str());
      ++failures;
    }

    /* 100000 opening parentheses, 100000 signs: refused by the nesting limit */
    if (expr_compile((std::string(100000, '(') + "1").c_str(), 1, program, error) != kExprErrArg) {
      std::printf("deep parentheses are not refused\n");
      ++failures;
    }
    if (expr_compile((std::string(100000, '-') + "1").c_str(), 1, program, error) != kExprErrArg) {
      std::printf("a long chain of signs is not refused\n");
      ++failures;
    }
  }
} // namespace

int main(int argc, char **argv)
{
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "grammar")
    grammar();
  else if (mode == "refusals")
    refusals();
  else if (mode == "limits")
    limits();
  else {
    std::printf("usage: expression_cases grammar|refusals|limits\n");
    return 2;
  }
  if (failures == 0)
    std::printf("ok\n");
  return failures == 0 ? 0 : 1;
}
