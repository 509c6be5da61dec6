from gen_adversarial_amd.experiments.alpha_learning.gradient_descent import main, parse_args  # noqa: F401

if __name__ == '__main__':
    main(parse_args())
