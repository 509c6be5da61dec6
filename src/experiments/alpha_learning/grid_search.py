from gen_adversarial_amd.experiments.alpha_learning.grid_search import main, parse_args, save_results  # noqa: F401

if __name__ == '__main__':
    main(parse_args())
