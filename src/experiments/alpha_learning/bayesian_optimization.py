from gen_adversarial_amd.experiments.alpha_learning.bayesian_optimization import main, parse_args  # noqa: F401

if __name__ == '__main__':
    main(parse_args())
